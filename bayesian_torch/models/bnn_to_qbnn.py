from bayesian_torch_amd.models.bnn_to_qbnn import bnn_to_qbnn, qbnn_linear_layer, qbnn_conv_layer, batch_norm_folding  # noqa: F401
