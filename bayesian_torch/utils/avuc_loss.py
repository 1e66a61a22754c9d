from bayesian_torch_amd.utils.avuc_loss import (AvULoss, AUAvULoss, entropy, predictive_entropy, mutual_information, eval_avu,  # noqa: F401
                                                accuracy_vs_uncertainty)
