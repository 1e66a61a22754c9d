"""Alias package: the reference's ``bayesian_torch.ao`` import path (served by bayesian_torch_amd.quantization)."""
