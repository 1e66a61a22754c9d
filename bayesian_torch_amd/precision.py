"""Contraction arithmetic of the fused forwards (``bt_set_contraction`` / ``bt_get_contraction``, env ``BT_CONTRACTION``).

    from bayesian_torch_amd import precision
    with precision.contraction("bf16"):          # inference at one bf16 MFMA term per K16 step
        logits, kl = mc_forward(model, x, S)

Names:
  "auto"    every eligible launch runs the exact three-piece bf16 split (6 product terms, fp32-level accuracy); the default
  "f32"     fp32 MFMA everywhere
  "bf16x2"  two pieces, 3 terms (~1e-5 relative), Reparameterization only
  "bf16"    operands rounded once to bf16 (nearest even), 1 term, fp32 accumulate: relative error <= 2^-8 per product. It serves the
            Reparameterization launches that "auto" gives to the general split, stem or direct kernel; everything else (Flipout,
            the fp32-MFMA launches, injected draws) runs as under "auto", and the KL is bit-identical to "auto"'s.

The knob is PROCESS-WIDE (not per thread, not per model) and is read at launch: a captured ``McGraph`` keeps the kernels it was
captured with, whatever the mode at replay. "bf16" is meant for inference: the backward does not know the mode, so a forward made
under autograd in it is differentiated by the fp32 backward of the unrounded function.
"""
import contextlib

NAMES = ("auto", "f32", "bf16x2", "bf16")   # index = the C mode


def _lib():
    from . import _lib as L   # (importing the package does not load the library; the first call here does)
    return L


def set_contraction(name):
    """Select the contraction arithmetic by name; ValueError for an unknown name."""
    if name not in NAMES:
        raise ValueError(f"unknown contraction {name!r}: one of {', '.join(NAMES)}")
    L = _lib()
    L.check(L.lib().bt_set_contraction(NAMES.index(name)))


def get_contraction():
    """Name of the mode in force (what was last set, else BT_CONTRACTION, else "auto")."""
    return NAMES[_lib().lib().bt_get_contraction()]


@contextlib.contextmanager
def contraction(name):
    """Run a block under ``name`` and restore the previous mode on exit, also when the block raises."""
    prev = get_contraction()
    set_contraction(name)
    try:
        yield
    finally:
        set_contraction(prev)
