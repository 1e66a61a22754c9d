from bayesian_torch_amd.quantization.quantize import convert, enable_prepare, observer_qparams, prepare  # noqa: F401
