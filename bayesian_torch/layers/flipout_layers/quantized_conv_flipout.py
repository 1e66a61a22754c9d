from bayesian_torch_amd.layers._quantized import QuantizedConv2dFlipout  # noqa: F401

__all__ = ["QuantizedConv2dFlipout"]
