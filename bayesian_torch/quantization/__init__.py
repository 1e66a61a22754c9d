from bayesian_torch_amd.quantization import convert, enable_prepare, observer_qparams, prepare  # noqa: F401
from bayesian_torch_amd.quantization import DeQuantStub, QActivation, QFunctional, QuantStub  # noqa: F401
