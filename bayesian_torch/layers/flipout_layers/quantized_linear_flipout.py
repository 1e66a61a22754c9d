from bayesian_torch_amd.layers._quantized import QuantizedLinearFlipout  # noqa: F401

__all__ = ["QuantizedLinearFlipout"]
