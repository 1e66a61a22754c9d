"""The body the two LSTM layers share: an LSTM cell unrolled over time whose input-to-hidden (``ih``) and hidden-to-hidden (``hh``) maps
are two Bayesian Linear layers, a fresh weight draw per time step and per map -- reference ``layers/variational_layers/rnn_variational.py:45-153``
and ``layers/flipout_layers/rnn_flipout.py:45-153``. Both maps run on the fused linear kernel.

``set_lstm_path`` chooses what runs between them:

``"torch"`` (default)
    the gate arithmetic is plain torch -- an add, four slices, five activations, three multiplies, an add and two list appends per step --
    and every step's two Linear calls ask for their KL term. Launch for launch what this layer has always done.

``"fused"``
    ONE launch of the LSTM cell kernel per step (csrc/bt_lstm.hip: bt_lstm_cell_fwd). Without grad it writes h_t and c_t straight into
    time-major sequence storage, from which ``hh`` reads h_{t-1} with no copy; one re-layout at the end gives [batch, time, features].
    Under grad the cell is one ``autograd.LSTMCell`` per step (forward launch that saves the activated gates, backward launch of the
    closed form). The KL term of each map is taken ONCE per forward -- from step 0's call or from the model-level pack check -- and
    steps 1 .. T-1 launch without a KL sweep; ``forward(return_kl=True)`` returns T * (KL_ih + KL_hh), the value of the reference's
    per-step sum.

Both paths batch MC samples: inside ``mc_samples(S, B)`` X has B rows (shared by the samples) or S * B rows (stacked, sample-major) and
``hidden_seq`` / ``c_ts`` come back as [S * B, T, H]; every step and every map draws once per sample. The default initial state is
shared (``h`` goes to ``hh`` as a shared input, ``c`` is broadcast); a supplied one has B or S * B rows. Under a context that collects KL
terms the layer contributes KL_ih and KL_hh TWICE, whatever T is: ``get_kl_loss``, like the reference's, counts an LSTM's maps through the
LSTM module and again as its children, and ``mc_forward``'s sum then equals it.
"""
import os

import torch

from .. import mc
from .. import functional as F
from .base_variational_layer import BaseVariationalLayer_

LSTM_PATHS = ("torch", "fused")


def _check_lstm_path(name, what):
    if name not in LSTM_PATHS:
        raise ValueError(f"{what}: expected one of {LSTM_PATHS}, got {name!r}")
    return name


_lstm_path = [_check_lstm_path(os.environ.get("BT_LSTM_PATH", "torch"), "BT_LSTM_PATH")]


def set_lstm_path(name):
    """What runs between the two Linear launches of an LSTM time step: "torch" (default) the gate arithmetic in torch ops, "fused" one
    launch of the LSTM cell kernel, with each map's KL taken once per forward (module docstring). Process-wide; also the environment
    variable BT_LSTM_PATH, read at import. Returns the previous setting."""
    prev, _lstm_path[0] = _lstm_path[0], _check_lstm_path(name, "set_lstm_path")
    return prev


def get_lstm_path():
    return _lstm_path[0]


class LSTMLayer(BaseVariationalLayer_):
    _linear = None      # the class of the two maps (the subclass's)

    def __init__(self, in_features, out_features, prior_mean=0, prior_variance=1, posterior_mu_init=0,
                 posterior_rho_init=-3.0, bias=True):
        super().__init__()
        self.in_features, self.out_features = in_features, out_features
        self.prior_mean, self.prior_variance = prior_mean, prior_variance
        self.posterior_mu_init, self.posterior_rho_init = (posterior_mu_init,), (posterior_rho_init,)
        self.bias = bias
        mk = lambda n_in: self._linear(in_features=n_in, out_features=4 * out_features, prior_mean=prior_mean,
                                       prior_variance=prior_variance, posterior_mu_init=posterior_mu_init,
                                       posterior_rho_init=posterior_rho_init, bias=bias)
        self.ih = mk(in_features)
        self.hh = mk(out_features)

    def kl_loss(self):
        return self.ih.kl_loss() + self.hh.kl_loss()

    def _initial_state(self, X, hidden_states, ctx):
        """(h, c) of step 0. Inside mc_samples(S, B) the default is ONE state of B rows shared by the samples; a supplied one has B or
        S * B rows."""
        n, hs = X.size(0), self.out_features
        if ctx is not None and n != ctx.batch and n != ctx.S * ctx.batch:
            raise RuntimeError(f"inside mc_samples(S={ctx.S}, batch={ctx.batch}) {type(self).__name__} got X of shape {tuple(X.shape)}")
        if hidden_states is None:
            rows = n if ctx is None else ctx.batch
            return torch.zeros(rows, hs, device=X.device), torch.zeros(rows, hs, device=X.device)
        h, c = hidden_states
        if ctx is not None:
            for what, t in (("h", h), ("c", c)):
                if t.dim() != 2 or t.shape[0] not in (ctx.batch, ctx.S * ctx.batch) or t.shape[1] != hs:
                    raise RuntimeError(f"inside mc_samples(S={ctx.S}, batch={ctx.batch}) hidden_states {what} must be [{ctx.batch}, {hs}] or "
                                       f"[{ctx.S * ctx.batch}, {hs}], got {tuple(t.shape)}")
        return h, c

    def forward(self, X, hidden_states=None, return_kl=True):
        if self.dnn_to_bnn_flag:
            return_kl = False
        ctx = mc.current()
        collect = ctx is not None and ctx.collect_kl
        n_kls = len(ctx.kls) if collect else 0
        h, c = self._initial_state(X, hidden_states, ctx)
        S, rows = (1, X.size(0)) if ctx is None else (ctx.S, ctx.S * ctx.batch)      # rows of the outputs: the samples' batches, sample-major
        if _lstm_path[0] == "fused":
            hidden_seq, c_ts, kl, kl_maps = self._forward_fused(X, h, c, rows, return_kl or collect)
        else:
            hidden_seq, c_ts, kl, kl_maps = self._forward_torch(X, h, c, S)
        if collect:      # each map once through this module and once as its child, as get_kl_loss counts them -- not once per step
            del ctx.kls[n_kls:]
            if kl_maps is not None:
                ctx.kls.extend(kl_maps * 2)
        if return_kl:
            return hidden_seq, (hidden_seq, c_ts), kl
        return hidden_seq, (hidden_seq, c_ts)

    def _forward_torch(self, X, h, c, S):
        """The reference's loop: every step's two calls ask for their KL term, whoever reads it."""
        hs = self.out_features
        kl, kl_maps = 0, None
        hidden, cells = [], []
        for t in range(X.size(1)):
            a, kl_a = self.ih(X[:, t, :])
            b, kl_b = self.hh(h)
            gates = a + b
            kl = kl + kl_a + kl_b
            if kl_maps is None:
                kl_maps = [kl_a, kl_b]
            i_t, f_t = torch.sigmoid(gates[:, :hs]), torch.sigmoid(gates[:, hs:2 * hs])
            g_t, o_t = torch.tanh(gates[:, 2 * hs:3 * hs]), torch.sigmoid(gates[:, 3 * hs:])
            if c.shape[0] != gates.shape[0]:      # a state shared by the S samples of an MC batch
                c = c.repeat(S, 1)
            c = f_t * c + i_t * g_t
            h = o_t * torch.tanh(c)
            hidden.append(h)
            cells.append(c)
        hidden_seq = torch.stack(hidden, dim=1).contiguous()      # [batch, time, features]
        c_ts = torch.stack(cells, dim=1).contiguous()
        return hidden_seq, c_ts, kl, kl_maps

    def _maps(self, x_t, h, want_kl):
        """One step's two Linear launches -> (a, b, [KL_ih, KL_hh] or None). Without ``want_kl`` neither sweeps its KL term nor hands one
        to a collecting context."""
        if want_kl:
            a, kl_a = self.ih(x_t)
            b, kl_b = self.hh(h)
            return a, b, [kl_a, kl_b]
        self.ih._kl_muted = self.hh._kl_muted = True
        try:
            return self.ih(x_t, return_kl=False), self.hh(h, return_kl=False), None
        finally:
            self.ih._kl_muted = self.hh._kl_muted = False

    def _forward_fused(self, X, h, c, rows, want_kl):
        hs, steps = self.out_features, X.size(1)
        if steps == 0:
            raise RuntimeError(f"{type(self).__name__}: X has no time steps: {tuple(X.shape)}")
        Xt = X.transpose(0, 1).contiguous()      # [time, batch, features]: every step's input is a contiguous slab
        needs_grad = torch.is_grad_enabled() and (X.requires_grad or h.requires_grad or c.requires_grad or any(p.requires_grad for p in self.parameters()))
        kl_maps = None
        if needs_grad:
            from ..autograd import LSTMCell
            hidden, cells = [], []
            for t in range(steps):
                a, b, k = self._maps(Xt[t], h, want_kl and t == 0)
                kl_maps = k if t == 0 else kl_maps
                h, c = LSTMCell.apply(a, b, c)
                hidden.append(h)
                cells.append(c)
            hidden_seq, c_ts = torch.stack(hidden, dim=1).contiguous(), torch.stack(cells, dim=1).contiguous()
        else:
            hbuf = torch.empty((steps, rows, hs), dtype=torch.float32, device=X.device)      # time-major: hh reads slab t - 1 as it lies
            cbuf = torch.empty((steps, rows, hs), dtype=torch.float32, device=X.device)
            for t in range(steps):
                a, b, k = self._maps(Xt[t], h, want_kl and t == 0)
                kl_maps = k if t == 0 else kl_maps
                h, c, _ = F.lstm_cell_fwd(a, b, c, h_out=hbuf[t], c_out=cbuf[t])
            hidden_seq, c_ts = hbuf.transpose(0, 1).contiguous(), cbuf.transpose(0, 1).contiguous()
        kl = None if kl_maps is None else steps * (kl_maps[0] + kl_maps[1])
        return hidden_seq, c_ts, kl, kl_maps
