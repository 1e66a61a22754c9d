from bayesian_torch_amd.layers.variational_layers.conv_variational import *  # noqa: F401,F403
from bayesian_torch_amd.layers.variational_layers.conv_variational import Conv2dReparameterization_Multivariate  # noqa: F401,E402  (not in __all__, as in the reference)
