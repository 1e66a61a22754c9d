"""Every forward-kernel instantiation the library holds meets the fp64 oracle: one test id per kernel name of the instantiation ledger
(tests/golden/instantiation_cases.json; tests/test_instantiation_ledger_host.py holds the ledger to the library's symbol table).

Per row, for its ``min`` case and its ``ragged`` (or ``edge``) case alike (tests/_inst_cases.py): one launch through the public
functional entry point with the row's knobs, the kernel name after the real launch equal to the row's -- a shape that drifts to
another kernel fails, it does not silently test something else --, the result inside intact guard bands with every element written,
and every sample and every output element against oracle/bt_oracle.py in float64 on the draws that were used (on-chip draws
regenerated from the launch's coordinates, supplied draws the supplied ones, the pool epilogue as max_pool2d(3, 2, 1) of the oracle's
output). The judgement is the one the project already applies to the variant: rtol 1e-4 / atol 1e-5 max|ref| for the fp32 and
bf16x3 kernels; for bf16x1 the oracle on operands rounded once to bf16 at that tolerance and test_gpu_bf16_mode.py's magnitude bound
with its short-K rule; for bf16x2 the documented window of test_three_term_split_is_opt_in_and_coarser; for the low-rank rows
tests/_lowrank_ref.py's reference; for the observer rows the calibration case module's reference and tolerances."""
import pytest
import torch

import _inst_cases as IC

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", sorted(IC.ledger()["rows"]))
def test_instantiation_meets_the_oracle(name):
    row = IC.ledger()["rows"][name]
    dev = torch.device("cuda", torch.cuda.current_device())
    for tag, c in IC.cases_of(row):
        ran = IC.run_case(name, tag, c, dev)
        print(f"{name} [{tag}]: {c['macs']} MACs, ran {ran}")
