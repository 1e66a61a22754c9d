from .conv_flipout import *
from .linear_flipout import *
from .rnn_flipout import *
from .._quantized import QuantizedConv2dFlipout, QuantizedLinearFlipout
