"""Post-training INT8 quantisation of a Bayesian model: ``prepare`` -> calibration batches -> ``convert`` (quantize.py); u8
activations between the converted layers (qact.py)."""
from . import qact  # noqa: F401
from .qact import DeQuantStub, QActivation, QFunctional, QuantStub  # noqa: F401
from .quantize import convert, enable_prepare, observer_qparams, prepare  # noqa: F401

__all__ = ["prepare", "convert", "enable_prepare", "observer_qparams", "qact", "QActivation", "QuantStub", "DeQuantStub", "QFunctional"]
