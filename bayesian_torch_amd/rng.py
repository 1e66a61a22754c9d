"""Draw management for the fused kernels.

Two modes (``set_mode``):

``"philox"`` (default, the product path)
    eps and the Flipout signs are generated on chip from counter coordinates
    ``(seed, call, layer_id, tensor, global sample id, element)``; nothing weight-sized is
    written to or read from HBM for the draw.  ``layer.eps_*`` buffers are NOT updated
    (``layer.materialize_last_draw()`` regenerates them on demand from the same counters).

``"torch"`` (parity mode)
    the draw is made exactly where the reference makes it -- ``eps.normal_()`` /
    ``uniform_(-1, 1).sign()`` on the input's device with torch's default generator, in the
    reference's draw order (linear_variational.py:164-174, conv_flipout.py:385-402) -- and the
    kernels READ it.  ``layer.eps_*`` hold the last draw as in the reference.

Where a supplied draw runs (``set_inject_path``; ``inject_draw`` and ``"torch"`` mode alike):

``"general"`` (default)
    the fp32 general kernel reads the draw in its natural layout.

``"split"``
    Reparameterization layers under ``torch.no_grad()``: the draw is re-laid into the packed parameters' layout
    (``bt_pack_eps``) and read by the injected instantiations of the split-precision (bf16x3) kernels -- the kernels an
    on-chip launch runs, so a replayed on-chip draw reproduces that launch's output bit for bit.  A launch no split
    flavour takes (and every Flipout layer) runs as under ``"general"``.  Environment: ``BT_INJECT_PATH``, read once.

The seed defaults to ``torch.initial_seed()``; ``call`` advances once per layer forward and
restarts whenever the seed changes, so ``torch.manual_seed(s)`` makes a run reproducible.
"""
import os
import threading

import torch

_state = threading.local()
_layer_counter = [0]
_mode = ["philox"]


def set_mode(mode):
    if mode not in ("philox", "torch"):
        raise ValueError("rng mode must be 'philox' or 'torch'")
    _mode[0] = mode


def get_mode():
    return _mode[0]


_INJECT_PATHS = ("general", "split")


def _check_inject_path(path, what):
    if path not in _INJECT_PATHS:
        raise ValueError(f"{what} must be 'general' or 'split', got {path!r}")
    return path


_inject_path = [_check_inject_path(os.environ.get("BT_INJECT_PATH", "general"), "BT_INJECT_PATH")]


def set_inject_path(path):
    _inject_path[0] = _check_inject_path(path, "inject path")


def get_inject_path():
    return _inject_path[0]


def new_layer_id():
    _layer_counter[0] += 1
    return _layer_counter[0]


def assign_layer_ids(model, first=1):
    """Number the Bayesian layers of ``model`` by position (``model.modules()`` order): layer_id is the RNG coordinate
    that separates the layers' draw streams, so two copies of a model (``copy.deepcopy``, or the same architecture built
    twice in any order) draw identically for the same (seed, call).  ``dnn_to_bnn`` calls this; call it yourself for a
    hand-assembled model of ``bayesian_torch_amd.layers`` modules if construction-order independence matters."""
    n = first
    for m in model.modules():
        if hasattr(m, "_layer_id") and (hasattr(m, "_kl_segments") or getattr(m, "_rng_layer", False)):
            m._layer_id = n
            n += 1
    return n - first


def manual_seed(seed):
    """Pin the Philox seed explicitly (otherwise torch.initial_seed() is followed)."""
    _state.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    _state.pinned = True
    _state.call = 0


def _sync():
    if not getattr(_state, "pinned", False):
        s = torch.initial_seed() & 0xFFFFFFFFFFFFFFFF
        if getattr(_state, "seed", None) != s:
            _state.seed = s
            _state.call = 0


def seed():
    _sync()
    return _state.seed


def next_call():
    _sync()
    c = getattr(_state, "call", 0)
    _state.call = (c + 1) & 0xFFFFFFFF
    return c


def peek_call():
    _sync()
    return getattr(_state, "call", 0)


def set_call(c):
    _sync()
    _state.call = int(c) & 0xFFFFFFFF
