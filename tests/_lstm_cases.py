"""Inputs and references shared by test_lstm_fused_host.py (CPU) and test_gpu_lstm_fused.py (GPU). A plain module: no fixtures, no
pytest hooks. Every input is generated from a seed here; every reference is the torch gate arithmetic of oracle/bt_oracle.py's
``lstm_ref`` (sigmoid / tanh of the four H-wide slices of a + b, c = f c_prev + i g, h = o tanh c) and torch autograd of it -- never the
closed form of csrc/bt_lstm.hip, which is what the tests hold to it."""
import functools

import torch

# The kernels may be this many times worse than CPU torch's float32 evaluation of the same arithmetic on the same inputs: they chain
# the hardware's exp2 and rcp (about 1 ulp each) where torch calls libm. Same reasoning as _grad_cases.KL_FACTOR.
FACTOR = 8.0

# (id, H, rows, |z| up to, c_rows or None = rows, what else the row does)
#   H 5 / 130: no whole quads per row -> the element-wise form (130: a two-unit tail behind 32 quads); 257 rows x 16 quads: more than
#   one block of 256 threads; |z| 30 / 90: saturated gates (float32 exp overflows from 88.7); c_rows 2 of 6 rows: a state shared by
#   three samples; slab: h / c written into time slab 1 of a [4, 3, 64] buffer (row stride 192).
CELL_ROWS = [
    ("h5", 5, 3, 4.0, None, None),
    ("h64x257", 64, 257, 4.0, None, None),
    ("h130z30", 130, 33, 30.0, None, None),
    ("h8z90", 8, 64, 90.0, None, "pm90"),
    ("h64shared-c", 64, 6, 4.0, 2, None),
    ("h64slab", 64, 4, 4.0, None, "slab"),
    ("h64no-b", 64, 5, 4.0, None, "no_b"),
    ("h64no-grad-h", 64, 5, 4.0, None, "no_gh"),
    ("h64no-grad-c", 64, 5, 4.0, None, "no_gc"),
]
CELL_IDS = [r[0] for r in CELL_ROWS]
OUTPUTS = ("h", "c", "dz", "dc_prev")


@functools.lru_cache(maxsize=None)
def cell_inputs(i):
    """Row i's fixed float32 inputs: a, b [rows, 4H] with |a + b| <= zmax (b None for the no-b row), c_prev [c_rows, H], and the
    upstream grad_h / grad_c [rows, H] (None where the row leaves one out). The +-90 row: z is exactly +90 on row 0 and -90 on row 1."""
    name, H, rows, zmax, c_rows, special = CELL_ROWS[i]
    gen = torch.Generator().manual_seed(4100 + i)
    u = lambda *shape: torch.rand(*shape, generator=gen) * 2 - 1
    a, b = u(rows, 4 * H) * (zmax / 2), u(rows, 4 * H) * (zmax / 2)
    if special == "pm90":
        a[0], b[0], a[1], b[1] = 45.0, 45.0, -45.0, -45.0
    if special == "no_b":
        a, b = a + b, None
    c_prev = torch.randn(c_rows or rows, H, generator=gen)
    gh, gc = torch.randn(rows, H, generator=gen), torch.randn(rows, H, generator=gen)
    return dict(a=a, b=b, c_prev=c_prev, grad_h=None if special == "no_gh" else gh, grad_c=None if special == "no_gc" else gc, H=H, rows=rows,
                special=special)


def gates(z, H):
    """The reference's gate arithmetic (oracle lstm_ref) -> i, f, g, o."""
    return torch.sigmoid(z[:, :H]), torch.sigmoid(z[:, H:2 * H]), torch.tanh(z[:, 2 * H:3 * H]), torch.sigmoid(z[:, 3 * H:])


def cell_ref(t, dtype):
    """-> dict(h, c, act, dz, dc_prev) of the inputs ``t`` by the torch gate arithmetic and its autograd in ``dtype`` on the CPU.
    dc_prev is per ROW, as the kernel returns it (a shared c_prev is expanded to the rows before it becomes a leaf)."""
    H, rows = t["H"], t["rows"]
    cv = lambda v: v.detach().cpu().to(dtype)
    a = cv(t["a"]).requires_grad_(True)
    z = a if t["b"] is None else a + cv(t["b"])
    cp = cv(t["c_prev"])
    cp = cp.repeat(rows // cp.shape[0], 1).requires_grad_(True)
    i, f, g, o = gates(z, H)
    c = f * cp + i * g
    h = o * torch.tanh(c)
    loss = 0
    if t["grad_h"] is not None:
        loss = loss + (h * cv(t["grad_h"])).sum()
    if t["grad_c"] is not None:
        loss = loss + (c * cv(t["grad_c"])).sum()
    dz, dcp = torch.autograd.grad(loss, (a, cp))
    return dict(h=h.detach(), c=c.detach(), act=torch.cat([i, f, g, o], 1).detach(), dz=dz, dc_prev=dcp)


def closed_form(t, dtype):
    """The backward as csrc/bt_lstm.hip states it, on the reference's own activations in ``dtype`` -> (dz, dc_prev)."""
    r = cell_ref(t, dtype)
    H, rows = t["H"], t["rows"]
    i, f, g, o = (r["act"][:, k * H:(k + 1) * H] for k in range(4))
    zero = torch.zeros(rows, H, dtype=dtype)
    gh = zero if t["grad_h"] is None else t["grad_h"].to(dtype)
    gc = zero if t["grad_c"] is None else t["grad_c"].to(dtype)
    cp = t["c_prev"].to(dtype).repeat(rows // t["c_prev"].shape[0], 1)
    tc = torch.tanh(r["c"])
    dc = gc + gh * o * (1 - tc * tc)
    return torch.cat([dc * g * i * (1 - i), dc * cp * f * (1 - f), dc * i * (1 - g * g), gh * tc * o * (1 - o)], 1), dc * f


def metric(got, ref64):
    """max |got - ref64| / (1 + |ref64|), in float64; nan when anything is not finite (no limit admits it)."""
    got, ref64 = got.detach().double().cpu(), ref64.detach().double().cpu()
    assert got.shape == ref64.shape, (got.shape, ref64.shape)
    e = (got - ref64).abs() / (1 + ref64.abs())
    return float("nan") if not bool(torch.isfinite(e).all()) else float(e.max())


@functools.lru_cache(maxsize=None)
def cell_row(i):
    """Row i -> dict(inputs, ref64, ref32, ref32_err {output: metric}, limit {output: FACTOR * metric}). Computed once."""
    t = cell_inputs(i)
    ref64, ref32 = cell_ref(t, torch.float64), cell_ref(t, torch.float32)
    err = {k: metric(ref32[k], ref64[k]) for k in OUTPUTS}
    return dict(inputs=t, ref64=ref64, ref32=ref32, ref32_err=err, limit={k: FACTOR * v for k, v in err.items()})


# ------------------------------------------------------------------------------------------------ layers
def spread_rho(lstm, seed=3):
    """rho spread out, so that sigma * eps is not a small correction of mu (a wrong or missing draw must show)."""
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for lin in (lstm.ih, lstm.hh):
            for p in (lin.rho_weight, lin.rho_bias):
                p.copy_(torch.rand(p.shape, generator=gen) * 2 - 2.5)
    return lstm


def mc_x(S, B, T, n_in, stacked, seed=5):
    gen = torch.Generator().manual_seed(seed)
    return torch.randn((S * B if stacked else B), T, n_in, generator=gen)


class LSTMHead(torch.nn.Module):
    """nn.LSTM(7, 5, batch_first=True) and a Linear head on the last step: what dnn_to_bnn converts in the model tests."""

    def __init__(self, n_in=7, hidden=5, classes=3):
        super().__init__()
        self.lstm = torch.nn.LSTM(n_in, hidden, batch_first=True)
        self.head = torch.nn.Linear(hidden, classes)

    def forward(self, x):
        out = self.lstm(x)
        return self.head(out[0][:, -1])
