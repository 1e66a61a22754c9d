"""Post-training INT8 quantisation of a Bayesian model: ``prepare`` -> calibration batches -> ``convert`` (quantize.py)."""
from .quantize import convert, enable_prepare, observer_qparams, prepare  # noqa: F401

__all__ = ["prepare", "convert", "enable_prepare", "observer_qparams"]
