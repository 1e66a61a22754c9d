from bayesian_torch_amd.quantization.qact import *  # noqa: F401,F403
from bayesian_torch_amd.quantization.qact import __all__  # noqa: F401
