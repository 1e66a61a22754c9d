from bayesian_torch_amd.layers.variational_layers.hiearchial_variational_layers import (  # noqa: F401
    HYPO_A, HYPO_B, Conv2dReparameterizationHierarchical, Conv2dReparameterizationHierarchical_Weightwise,
    LinearReparameterizationHierarchical, LinearReparameterizationHierarchical_Weightwise)
