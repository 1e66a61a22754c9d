from .flipout_layers import *
from .variational_layers import *
from .base_variational_layer import *
from ._family import get_conv3d_path, get_transpose_path, set_conv3d_path, set_transpose_path
from ._lstm import get_lstm_path, set_lstm_path
from ._lowrank import get_lowrank_train_path, set_lowrank_train_path
