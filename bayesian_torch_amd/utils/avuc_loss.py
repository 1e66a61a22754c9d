"""Accuracy versus uncertainty calibration (AvUC) -- drop-in for reference ``utils/avuc_loss.py`` (Krishnan & Tickoo, NeurIPS 2020).

``AvULoss`` and ``AUAvULoss`` run on the HIP kernels of csrc/bt_avu.hip: a row pass, a one-workgroup finish pass and
one backward launch, with no read on the host -- the reference walks the batch in a Python loop of ``.item()`` calls. What differs
from the reference, on purpose:

- ``AUAvULoss.forward`` works (the reference hands a list of tensors to ``sklearn.metrics.auc`` and fails); its value is the
  trapezoid of AvU over ``np.linspace(0, 1, 21)``, what ``auc`` computes, and it is differentiable.
- The first and last thresholds are the batch's smallest and largest uncertainty exactly (the reference's last one misses the
  largest by a rounding of ``umin + 1.0 * (umax - umin)`` in about half of all batches).
- ``type=1`` (model uncertainty) takes Monte Carlo logits ``[S, B, C]``, as ``mc.mc_forward`` returns them; on ``[B, C]`` logits it
  raises ``ValueError`` (the reference raises ``IndexError`` there). ``[S, B, C]`` logits are accepted for ``type=0`` as well: the
  prediction, the confidence and the entropy are then those of the mean of the samples' softmax.
- The threshold may be a device tensor, so a step under ``mc.TrainGraph`` can change it between replays.

The module-level functions are the reference's numpy metrics (1e-15 guards), vectorised on the host."""
import numpy as np
import torch
from torch import nn

from .. import autograd as A

_EPS = 1e-10


def _mc_logits(logits, type):
    if type not in (0, 1):
        raise ValueError(f"type must be 0 (predictive uncertainty) or 1 (model uncertainty), got {type!r}")
    if logits.dim() == 2:
        if type == 1:
            raise ValueError("type=1 (model uncertainty) is the spread over Monte Carlo samples: pass the MC form of the logits, "
                             "[S, B, C] with S > 1 (mc.mc_forward returns it), not [B, C]")
        return logits.unsqueeze(0)
    if logits.dim() != 3:
        raise ValueError(f"logits are [B, C], or [S, B, C] in the MC form; got {tuple(logits.shape)}")
    if type == 1 and logits.shape[0] < 2:
        raise ValueError("type=1 (model uncertainty) needs S > 1 samples in the MC form [S, B, C]")
    return logits


class _AvUBase(nn.Module):
    def __init__(self, beta=1):
        super().__init__()
        self.beta = beta
        self.eps = _EPS
        self.last_stats = None

    def entropy(self, prob):
        return -1 * torch.sum(prob * torch.log(prob + self.eps), dim=-1)

    def expected_entropy(self, mc_preds):
        return torch.mean(self.entropy(mc_preds), dim=0)

    def predictive_uncertainty(self, mc_preds):
        """Entropy of the mean of the predictive distribution obtained from Monte Carlo sampling."""
        return self.entropy(torch.mean(mc_preds, dim=0))

    def model_uncertainty(self, mc_preds):
        """Entropy of the mean of the predictive distribution minus the mean of the samples' entropies."""
        return self.entropy(torch.mean(mc_preds, dim=0)) - self.expected_entropy(mc_preds)

    def accuracy_vs_uncertainty(self, prediction, true_label, uncertainty, optimal_threshold):
        """The AvU metric (counts, not the soft sums) as a [1] tensor on the labels' device; nothing is printed."""
        acc = true_label == prediction
        cert = uncertainty <= optimal_threshold
        n = torch.stack([(acc & cert).sum(), (acc & ~cert).sum(), (~acc & cert).sum(), (~acc & ~cert).sum()]).to(torch.float32)
        return ((n[0] + n[3]) / n.sum()).reshape(1)

    def _run(self, logits, labels, threshold, type, T):
        z = _mc_logits(logits, type)
        if not z.is_cuda:
            raise RuntimeError(f"logits are on {z.device}: bayesian_torch_amd runs on a HIP (MI355X) device only; there is no CPU "
                               "implementation of this loss")
        if T == 1:
            if torch.is_tensor(threshold):
                threshold = threshold.detach().to(device=z.device, dtype=torch.float32).reshape(1)
            else:
                threshold = torch.full((1,), float(threshold), dtype=torch.float32, device=z.device)
        stats = {}
        loss, v = A.AvU.apply(z, labels, threshold, type, T, float(self.beta), stats)
        self.last_stats = stats
        return loss, v


class AvULoss(_AvUBase):
    """Accuracy versus uncertainty loss against a given uncertainty threshold. ``forward(logits, labels,
    optimal_uncertainty_threshold, type=0)`` -> loss [1]. The threshold is a Python number or a one-element device tensor (never read
    back). After a call ``last_stats`` holds device tensors: sums [1, 4] (n_ac, n_au, n_ic, n_iu), counts [1, 4], thresholds [1],
    and per row confidence, uncertainty, tanh_uncertainty, pred, acc."""

    def forward(self, logits, labels, optimal_uncertainty_threshold, type=0):
        return self._run(logits, labels, optimal_uncertainty_threshold, type, 1)[0]


class AUAvULoss(_AvUBase):
    """Accuracy versus uncertainty loss without a threshold: minus the log of the area under AvU over 21 thresholds between the
    batch's smallest and largest uncertainty. ``forward(logits, labels, type=0)`` -> (loss [1], auc_avu [1]); ``last_stats`` as
    ``AvULoss`` with 21 rows."""

    def forward(self, logits, labels, type=0):
        return self._run(logits, labels, None, type, 21)

    def auc_avu(self, logits, labels, unc):
        """Area under AvU for a given per-row uncertainty ``unc`` [B] and [B, C] logits, as a [1] tensor (torch ops on the tensors'
        device, no gradient): the reference's method with the end thresholds exact."""
        with torch.no_grad():
            probs = torch.softmax(logits, dim=1)
            conf, pred = torch.max(probs, 1)
            x = torch.from_numpy(np.linspace(0, 1, 21)).to(unc.device)
            u = unc.to(torch.float64)
            umin, umax = u.min(), u.max()
            th = umin + x * (umax - umin)
            th[0], th[-1] = umin, umax
            cert = u[None, :] <= th[:, None]
            acc = (pred == labels)[None, :]
            t = torch.tanh(unc)
            hi, lo = 1 - t, t
            n_ac = (torch.where(acc & cert, conf * hi, 0.0)).sum(1)
            n_au = (torch.where(acc & ~cert, conf * lo, 0.0)).sum(1)
            n_ic = (torch.where(~acc & cert, (1 - conf) * hi, 0.0)).sum(1)
            n_iu = (torch.where(~acc & ~cert, (1 - conf) * lo, 0.0)).sum(1)
            avu = ((n_ac + n_iu) / (n_ac + n_au + n_ic + n_iu + self.eps)).to(torch.float64)
            return torch.trapezoid(avu, x).to(torch.float32).reshape(1)


# ---- numpy metrics (reference utils/avuc_loss.py:370-443; host side) ----------------------------------------------------------------
def entropy(prob):
    return -1 * np.sum(prob * np.log(prob + 1e-15), axis=-1)


def predictive_entropy(mc_preds):
    """Entropy of the mean of the predictive distribution obtained from Monte Carlo sampling."""
    return entropy(np.mean(mc_preds, axis=0))


def mutual_information(mc_preds):
    """Entropy of the mean of the predictive distribution minus the mean of the samples' entropies."""
    return entropy(np.mean(mc_preds, axis=0)) - np.mean(entropy(mc_preds), axis=0)


def _counts(pred_label, true_label, uncertainty, th):
    """(n_ac, n_au, n_ic, n_iu) for every threshold of ``th`` (any shape): rows [N] against thresholds [..., 1]."""
    acc = np.asarray(true_label) == np.asarray(pred_label)
    cert = np.asarray(uncertainty) <= np.asarray(th)[..., None]
    unc = np.asarray(uncertainty) > np.asarray(th)[..., None]     # (a NaN uncertainty is in neither class, as in the reference)
    return (acc & cert).sum(-1), (acc & unc).sum(-1), (~acc & cert).sum(-1), (~acc & unc).sum(-1)


def eval_avu(pred_label, true_label, uncertainty):
    """AvU at 21 uncertainty thresholds between the smallest and the largest uncertainty -> (avu [21], thresholds [21])."""
    t_list = np.linspace(0, 1, 21)
    umin = np.amin(uncertainty, axis=0)
    umax = np.amax(uncertainty, axis=0)
    u_th = np.asarray([umin + (t * (umax - umin)) for t in t_list])
    n_ac, n_au, n_ic, n_iu = _counts(pred_label, true_label, uncertainty, u_th)
    return (n_ac + n_iu) / (n_ac + n_au + n_ic + n_iu + 1e-15), u_th


def accuracy_vs_uncertainty(pred_label, true_label, uncertainty, optimal_threshold):
    n_ac, n_au, n_ic, n_iu = (int(n) for n in _counts(pred_label, true_label, uncertainty, optimal_threshold))
    return (n_ac + n_iu) / (n_ac + n_au + n_ic + n_iu)
