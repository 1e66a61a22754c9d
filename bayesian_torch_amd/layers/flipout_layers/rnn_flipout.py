"""``LSTMFlipout`` -- drop-in for reference ``layers/flipout_layers/rnn_flipout.py:45-153``: an LSTM cell unrolled over
time whose input-to-hidden and hidden-to-hidden maps are two ``LinearFlipout`` layers (a fresh weight draw per time
step and per map, as in the reference). Both maps run on the fused linear kernel; the gate arithmetic between them is plain torch by
default and one launch of the LSTM cell kernel per step under ``set_lstm_path("fused")``. The loop, MC batching and the KL wiring are the
body the two LSTM classes share: ``layers/_lstm.py``."""
from .._lstm import LSTMLayer
from .linear_flipout import LinearFlipout

__all__ = ["LSTMFlipout"]


class LSTMFlipout(LSTMLayer):
    _linear = LinearFlipout

    def __init__(self, in_features, out_features, prior_mean=0, prior_variance=1, posterior_mu_init=0,
                 posterior_rho_init=-3.0, bias=True):
        super().__init__(in_features, out_features, prior_mean, prior_variance, posterior_mu_init, posterior_rho_init, bias)
