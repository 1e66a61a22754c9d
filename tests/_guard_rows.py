"""The row table of the guard-band tests, and the plan-only seam that pins each row's launch without a GPU.  A plain module shared
by test_guard_host.py (CPU: the kernel every row plans, aligned and misaligned) and test_gpu_guard_bands.py (GPU: the same rows run).

A row: id -> dict(
  flip, kind ("conv" | "linear" | "updil"), geo = (Ci, Co, k, stride, pad, H, B) (Linear: Ci = In, Co = Out), S,
  stacked (x holds S batches), mode (bt_set_contraction), pool, res (a per-sample residual with the folded scale / shift / ReLU stage),
  bias, kl (want_kl with all four priors), nat (natural-layout supplied draws), packs (False: no packed parameters),
  walk (the stem's sample walk, planned from the device's CU count: the seam plans its one-sample twin),
  ops = the operands displaced on the GPU, each alone and all together at off 1, 2 and 3 ("out", every result buffer, is displaced
        for every row),
  aligned = the kernel name with every operand 16-byte aligned, together = with all of ``ops`` displaced,
  single = {operand: name} for every operand of ``ops`` + ("out",) whose displacement ALONE changes the name (a refusal: its text),
  info / together_info / single_info = the INFO_FIELDS of bt_last_launch_info of those launches (single_info: where it differs from
  the aligned launch's).)
Which rows owe the aligned launch's bits is read off the two names (test_gpu_guard_bands.same_family), never off a measured equality.
The geometries are the smallest that reach the instantiation: those of tests/golden/split_plans.txt / fp32_plans.txt shrunk to S <= 3."""
import ctypes as C
import os

P = 0x10000000          # any non-null, 16-byte aligned address (never dereferenced: bt_debug_plan_only)
UPDIL = (2, 2, 1, 2, 1, 2)


# The launch-info fields a row states (bt_last_launch_info): what shows, beyond the kernel's name, that the row reaches the tile it is
# there for -- row tiles, the tile's images x rows x columns, the tile counts (partial batch / channel tiles), the KL slices.
INFO_FIELDS = ("row_tiles", "t_NI", "t_R", "t_Wt", "m_tiles", "n_tiles", "kl_slices")


def _row(flip, kind, geo, S, ops=(), aligned=None, info=None, together=None, together_info=None, single=None, single_info=None, **kw):
    r = dict(flip=flip, kind=kind, geo=geo, S=S, stacked=False, mode=0, pool=False, res=False, bias=False, kl=False, nat=False, packs=True, walk=False,
             ops=tuple(ops), aligned=aligned, info=info, together=together, together_info=together_info, single=dict(single or {}),
             single_info=dict(single_info or {}))
    assert not set(kw) - set(r), kw
    r.update(kw)
    return r


def info_of(info):
    """The stated fields of a launch info dict, in INFO_FIELDS order."""
    return tuple(info[k] for k in INFO_FIELDS)


ROWS = {
    "g_xm1": _row(False, 'conv', (8, 32, 1, 1, 0, 1, 128), 1, ops=('x', 'mu_w', 'rho_w', 'prior_mu_w', 'prior_sigma_w', 'mu_b', 'rho_b', 'prior_mu_b', 'prior_sigma_b'), kl=True, bias=True,
             aligned="fused_split_kernel<64,128,bf16x3,6 terms,npw=8,xm=1>", info=(0, 128, 1, 1, 1, 1, 1),
             together="fused_split_kernel<64,128,bf16x3,6 terms,npw=8,xm=0>", together_info=(0, 128, 1, 1, 1, 1, 1),
             single={"x": "fused_split_kernel<64,128,bf16x3,6 terms,npw=8,xm=0>"},
             single_info={}),
    "g_xm2_img4": _row(False, 'conv', (8, 32, 1, 1, 0, 2, 32), 1, ops=('x', 'residual', 'post_scale', 'post_shift'), res=True,
             aligned="fused_split_kernel<64,128,bf16x3,6 terms,npw=8,xm=2>", info=(0, 32, 2, 2, 1, 1, 1),
             together="fused_split_kernel<64,128,bf16x3,6 terms,npw=8,xm=0>", together_info=(0, 32, 2, 2, 1, 1, 1),
             single={"x": "fused_split_kernel<64,128,bf16x3,6 terms,npw=8,xm=0>"},
             single_info={}),
    "g_xm3_256": _row(False, 'conv', (8, 256, 1, 1, 0, 4, 176), 3, ops=('x',),
             aligned="fused_split_kernel<64,256,bf16x3,6 terms,npw=8,xm=3>", info=(0, 16, 4, 4, 11, 4, 132),
             together="fused_split_kernel<64,256,bf16x3,6 terms,npw=8,xm=0>", together_info=(0, 16, 4, 4, 11, 4, 132),
             single={"x": "fused_split_kernel<64,256,bf16x3,6 terms,npw=8,xm=0>"},
             single_info={}),
    "g_xm3_512": _row(False, 'conv', (8, 256, 1, 1, 0, 8, 88), 3, ops=('x',),
             aligned="fused_split_kernel<64,512,bf16x3,6 terms,npw=4,xm=3>", info=(0, 8, 8, 8, 11, 4, 132),
             together="fused_split_kernel<64,512,bf16x3,6 terms,npw=4,xm=0>", together_info=(0, 8, 8, 8, 11, 4, 132),
             single={"x": "fused_split_kernel<64,512,bf16x3,6 terms,npw=4,xm=0>"},
             single_info={}),
    "g_xm4": _row(False, 'conv', (8, 256, 1, 2, 0, 8, 176), 3, ops=('x',),
             aligned="fused_split_kernel<64,256,bf16x3,6 terms,npw=8,xm=4>", info=(0, 16, 4, 4, 11, 4, 132),
             together="fused_split_kernel<64,256,bf16x3,6 terms,npw=8,xm=0>", together_info=(0, 16, 4, 4, 11, 4, 132),
             single={"x": "fused_split_kernel<64,256,bf16x3,6 terms,npw=8,xm=0>"},
             single_info={}),
    "g_flat": _row(False, 'conv', (8, 256, 3, 1, 1, 14, 16), 3, ops=('x',),
             aligned="fused_split_kernel<64,256,bf16x3,6 terms,npw=8,xm=3>", info=(0, 1, 14, 14, 16, 4, 192),
             together="fused_split_kernel<64,256,bf16x3,6 terms,npw=8,xm=0>", together_info=(0, 1, 14, 14, 16, 4, 192),
             single={"x": "fused_split_kernel<64,256,bf16x3,6 terms,npw=8,xm=0>"},
             single_info={}),
    "g_bn32": _row(False, 'conv', (8, 64, 1, 1, 0, 1, 128), 1, ops=('x',),
             aligned="fused_split_kernel<32,128,bf16x3,6 terms,npw=8,xm=1>", info=(0, 128, 1, 1, 1, 2, 2),
             together="fused_split_kernel<32,128,bf16x3,6 terms,npw=8,xm=0>", together_info=(0, 128, 1, 1, 1, 2, 2),
             single={"x": "fused_split_kernel<32,128,bf16x3,6 terms,npw=8,xm=0>"},
             single_info={}),
    "g_pbatch": _row(False, 'conv', (8, 32, 3, 1, 1, 1, 120), 1, ops=('x', 'mu_b', 'rho_b'), bias=True,
             aligned="fused_split_kernel<64,128,bf16x3,6 terms,npw=8,xm=1>", info=(0, 120, 1, 1, 1, 1, 1),
             together="fused_split_kernel<64,128,bf16x3,6 terms,npw=8,xm=0>", together_info=(0, 120, 1, 1, 1, 1, 1),
             single={"x": "fused_split_kernel<64,128,bf16x3,6 terms,npw=8,xm=0>"},
             single_info={}),
    "g_pchan": _row(False, 'conv', (72, 40, 3, 1, 1, 8, 8), 1, ops=('x', 'residual'), res=True, bias=True,
             aligned="fused_split_kernel<32,128,bf16x3,6 terms,npw=8,xm=0>", info=(0, 2, 8, 8, 4, 2, 8),
             together="fused_split_kernel<32,128,bf16x3,6 terms,npw=8,xm=0>", together_info=(0, 2, 8, 8, 4, 2, 8),
             single={},
             single_info={}),
    "g_rowtile": _row(False, 'conv', (8, 32, 3, 1, 1, 2, 64), 1, ops=('x', 'residual'), res=True,
             aligned="fused_split_kernel<64,128,bf16x3,6 terms,npw=8,xm=2>", info=(1, 64, 1, 2, 2, 1, 2),
             together="fused_split_kernel<64,128,bf16x3,6 terms,npw=8,xm=0>", together_info=(1, 64, 1, 2, 2, 1, 2),
             single={"x": "fused_split_kernel<64,128,bf16x3,6 terms,npw=8,xm=0>"},
             single_info={}),
    "f_xm1": _row(True, 'conv', (8, 32, 1, 1, 0, 1, 128), 1, ops=('x', 'mu_b', 'rho_b'), bias=True,
             aligned="fused_split_kernel<64,128,bf16x3,2x6 terms,flip,npw=8,xm=1>", info=(0, 128, 1, 1, 1, 1, 1),
             together="fused_split_kernel<64,128,bf16x3,2x6 terms,flip,npw=8,xm=0>", together_info=(0, 128, 1, 1, 1, 1, 1),
             single={"x": "fused_split_kernel<64,128,bf16x3,2x6 terms,flip,npw=8,xm=0>"},
             single_info={}),
    "f_256": _row(True, 'conv', (8, 256, 3, 1, 0, 16, 16), 3, ops=('x',),
             aligned="fused_split_kernel<64,256,bf16x3,2x6 terms,flip,npw=4,xm=3>", info=(0, 1, 14, 14, 16, 4, 192),
             together="fused_split_kernel<64,256,bf16x3,2x6 terms,flip,npw=4,xm=0>", together_info=(0, 1, 14, 14, 16, 4, 192),
             single={"x": "fused_split_kernel<64,256,bf16x3,2x6 terms,flip,npw=4,xm=0>"},
             single_info={}),
    "q_r": _row(False, 'conv', (3, 32, 1, 1, 0, 4, 32), 1, ops=('residual', 'x'), res=True,
             aligned="fused_split_quad_kernel<64,512,bf16x3,6 terms,pool=0>", info=(0, 32, 4, 4, 1, 1, 1),
             together="fused_fast_kernel<32,128,1,reparam,conv,notrans,inj=0,xmode=0,npw=8,pool=0>", together_info=(0, 8, 4, 4, 4, 1, 4),
             single={"residual": "fused_fast_kernel<32,128,1,reparam,conv,notrans,inj=0,xmode=1,npw=8,pool=0>",
                     "out": "fused_fast_kernel<32,128,1,reparam,conv,notrans,inj=0,xmode=1,npw=8,pool=0>"},
             single_info={"residual": (0, 8, 4, 4, 4, 1, 4), "out": (0, 8, 4, 4, 4, 1, 4)}),
    "q_r_pool": _row(False, 'conv', (3, 32, 1, 1, 0, 8, 32), 1, ops=('x',), pool=True,
             aligned="fused_split_quad_kernel<64,512,bf16x3,6 terms,pool=1>", info=(0, 8, 8, 8, 4, 1, 4),
             together="fused_split_quad_kernel<64,512,bf16x3,6 terms,pool=1>", together_info=(0, 8, 8, 8, 4, 1, 4),
             single={"out": "fused max-pool: this launch's tiles do not hold whole output images"},
             single_info={}),
    "q_walk": _row(False, 'conv', (3, 32, 1, 1, 0, 16, 512), 2, ops=('x',), pool=True, walk=True,
             aligned="fused_split_quad_kernel<64,512,bf16x3,6 terms,pool=1>", info=(0, 2, 16, 16, 256, 1, 256),
             together="fused_split_quad_kernel<64,512,bf16x3,6 terms,pool=1>", together_info=(0, 2, 16, 16, 256, 1, 256),
             single={"out": "fused max-pool: this launch's tiles do not hold whole output images"},
             single_info={}),
    "q_f": _row(True, 'conv', (3, 32, 1, 1, 0, 4, 32), 1, ops=('residual', 'x'), res=True,
             aligned="fused_split_quad_kernel<64,256,bf16x3,2x6 terms,flip,pool=0>", info=(0, 16, 4, 4, 2, 1, 2),
             together="fused_fast_kernel<32,128,1,flip,conv,notrans,inj=0,xmode=0,npw=8,pool=0>", together_info=(0, 8, 4, 4, 4, 1, 4),
             single={"residual": "fused_fast_kernel<32,128,1,flip,conv,notrans,inj=0,xmode=0,npw=8,pool=0>",
                     "out": "fused_fast_kernel<32,128,1,flip,conv,notrans,inj=0,xmode=0,npw=8,pool=0>"},
             single_info={"residual": (0, 8, 4, 4, 4, 1, 4), "out": (0, 8, 4, 4, 4, 1, 4)}),
    "q_f_pool": _row(True, 'conv', (3, 32, 1, 1, 0, 8, 4), 1, ops=('x',), pool=True,
             aligned="fused_split_quad_kernel<64,256,bf16x3,2x6 terms,flip,pool=1>", info=(0, 4, 8, 8, 1, 1, 1),
             together="fused_split_quad_kernel<64,256,bf16x3,2x6 terms,flip,pool=1>", together_info=(0, 4, 8, 8, 1, 1, 1),
             single={"out": "fused max-pool: this launch's tiles do not hold whole output images"},
             single_info={}),
    "d_res": _row(False, 'conv', (64, 32, 1, 1, 0, 2, 32), 1, ops=('x',),
             aligned="fused_split_direct_kernel<64,8x64,bf16x3,6 terms,resident W>", info=(0, 2, 1, 64, 1, 1, 1),
             together="fused_split_direct_kernel<64,8x64,bf16x3,6 terms,resident W>", together_info=(0, 2, 1, 64, 1, 1, 1),
             single={},
             single_info={}),
    "d_str": _row(False, 'conv', (512, 32, 1, 1, 0, 4, 256), 1, ops=('x',),
             aligned="fused_split_direct_kernel<64,8x64,bf16x3,6 terms,streamed W>", info=(0, 64, 1, 64, 1, 1, 1),
             together="fused_split_direct_kernel<64,8x64,bf16x3,6 terms,streamed W>", together_info=(0, 64, 1, 64, 1, 1, 1),
             single={},
             single_info={}),
    "s_64": _row(False, 'conv', (64, 32, 1, 1, 0, 1, 3), 2, ops=('mu_w', 'rho_w', 'prior_mu_w', 'prior_sigma_w', 'x', 'residual'), kl=True, res=True,
             aligned="fused_split_skinny_kernel<64,4x32,bf16x3,6 terms,split-K 64>", info=(0, 128, 1, 1, 1, 1, 2),
             together="fused_split_skinny_kernel<64,4x32,bf16x3,6 terms,split-K 64>", together_info=(0, 128, 1, 1, 1, 1, 2),
             single={},
             single_info={}),
    "s_128": _row(False, 'linear', (128, 36, 0, 0, 0, 0, 5), 2, ops=('x',),
             aligned="fused_split_skinny_kernel<64,4x32,bf16x3,6 terms,split-K 128>", info=(0, 128, 1, 1, 1, 1, 2),
             together="fused_split_skinny_kernel<64,4x32,bf16x3,6 terms,split-K 128>", together_info=(0, 128, 1, 1, 1, 1, 2),
             single={},
             single_info={}),
    "u_r": _row(False, 'updil', (8, 32, 3, 1, 0, 4, 4), 2, ops=('x',),
             aligned="fused_split_kernel<64,128,bf16x3,6 terms,npw=8,xm=5>", info=(0, 2, 8, 8, 2, 1, 4),
             together="fused_split_kernel<64,128,bf16x3,6 terms,npw=8,xm=5>", together_info=(0, 2, 8, 8, 2, 1, 4),
             single={},
             single_info={}),
    "u_f": _row(True, 'updil', (8, 32, 3, 1, 0, 4, 4), 2, ops=('x',),
             aligned="fused_split_kernel<64,128,bf16x3,2x6 terms,flip,npw=8,xm=5>", info=(0, 2, 8, 8, 2, 1, 4),
             together="fused_split_kernel<64,128,bf16x3,2x6 terms,flip,npw=8,xm=5>", together_info=(0, 2, 8, 8, 2, 1, 4),
             single={},
             single_info={}),
    "b_xm1": _row(False, 'conv', (8, 32, 1, 1, 0, 1, 128), 1, ops=('x',), mode=3,
             aligned="fused_split_kernel<64,128,bf16x1,1 terms,npw=8,xm=1>", info=(0, 128, 1, 1, 1, 1, 1),
             together="fused_split_kernel<64,128,bf16x1,1 terms,npw=8,xm=0>", together_info=(0, 128, 1, 1, 1, 1, 1),
             single={"x": "fused_split_kernel<64,128,bf16x1,1 terms,npw=8,xm=0>"},
             single_info={}),
    "p_cvec": _row(False, 'conv', (8, 32, 1, 1, 0, 1, 1), 1, ops=('x',), mode=1,
             aligned="fused_fast_kernel<128,32,4,reparam,conv,trans,inj=0,xmode=2,npw=8,pool=0>", info=(0, 32, 1, 1, 1, 1, 1),
             together="fused_fast_kernel<128,32,4,reparam,conv,trans,inj=0,xmode=0,npw=8,pool=0>", together_info=(0, 32, 1, 1, 1, 1, 1),
             single={"x": "fused_fast_kernel<128,32,4,reparam,conv,trans,inj=0,xmode=0,npw=8,pool=0>"},
             single_info={}),
    "p_rows": _row(False, 'conv', (3, 32, 1, 1, 0, 8, 4), 1, ops=('x',), mode=1,
             aligned="fused_fast_kernel<32,128,1,reparam,conv,trans,inj=0,xmode=1,npw=8,pool=0>", info=(0, 2, 8, 8, 2, 1, 2),
             together="fused_fast_kernel<32,128,1,reparam,conv,trans,inj=0,xmode=0,npw=8,pool=0>", together_info=(0, 2, 8, 8, 2, 1, 2),
             single={"x": "fused_fast_kernel<32,128,1,reparam,conv,trans,inj=0,xmode=0,npw=8,pool=0>",
                     "out": "fused_fast_kernel<32,128,1,reparam,conv,notrans,inj=0,xmode=1,npw=8,pool=0>"},
             single_info={}),
    "p_res": _row(False, 'conv', (3, 32, 1, 1, 0, 8, 4), 1, ops=('residual',), mode=1, res=True,
             aligned="fused_fast_kernel<32,128,1,reparam,conv,trans,inj=0,xmode=1,npw=8,pool=0>", info=(0, 2, 8, 8, 2, 1, 2),
             together="fused_fast_kernel<32,128,1,reparam,conv,notrans,inj=0,xmode=1,npw=8,pool=0>", together_info=(0, 2, 8, 8, 2, 1, 2),
             single={"residual": "fused_fast_kernel<32,128,1,reparam,conv,notrans,inj=0,xmode=1,npw=8,pool=0>",
                     "out": "fused_fast_kernel<32,128,1,reparam,conv,notrans,inj=0,xmode=1,npw=8,pool=0>"},
             single_info={}),
    "p_pool": _row(False, 'conv', (3, 32, 1, 1, 0, 4, 1), 1, ops=('x',), mode=1, pool=True,
             aligned="fused_fast_kernel<64,128,2,reparam,conv,trans,inj=0,xmode=1,npw=8,pool=1>", info=(0, 8, 4, 4, 1, 1, 1),
             together="fused max-pool: this launch's tiles do not hold whole output images", together_info=None,
             single={"x": "fused max-pool: this launch's tiles do not hold whole output images",
                     "out": "fused max-pool: this launch's tiles do not hold whole output images"},
             single_info={}),
    "p_oddx": _row(False, 'conv', (3, 32, 1, 1, 0, 5, 3), 2, ops=('x',), mode=1, stacked=True,
             aligned="fused_fast_kernel<32,128,1,reparam,conv,notrans,inj=0,xmode=0,npw=8,pool=0>", info=(0, 5, 5, 5, 1, 1, 2),
             together="fused_fast_kernel<32,128,1,reparam,conv,notrans,inj=0,xmode=0,npw=8,pool=0>", together_info=(0, 5, 5, 5, 1, 1, 2),
             single={},
             single_info={}),
    "p_general": _row(False, 'conv', (8, 32, 3, 1, 1, 8, 4), 1, ops=('mu_w', 'rho_w', 'prior_mu_w', 'prior_sigma_w', 'x'), mode=1, packs=False, kl=True,
             aligned="fused_fwd_kernel<32,128,1,reparam,conv,trans,inj=0>", info=(0, 0, 0, 0, 2, 1, 2),
             together="fused_fwd_kernel<32,128,1,reparam,conv,trans,inj=0>", together_info=(0, 0, 0, 0, 2, 1, 2),
             single={"out": "fused_fwd_kernel<32,128,1,reparam,conv,notrans,inj=0>"},
             single_info={}),
    "p_packs": _row(False, 'conv', (8, 32, 3, 1, 1, 8, 4), 1, ops=('mu_packed', 'sigma_packed'), mode=1,
             aligned="fused_fast_kernel<32,128,1,reparam,conv,trans,inj=0,xmode=1,npw=8,pool=0>", info=(0, 2, 8, 8, 2, 1, 2),
             together="fused_fwd_kernel<32,128,1,reparam,conv,trans,inj=0>", together_info=(0, 0, 0, 0, 2, 1, 2),
             single={"mu_packed": "fused_fwd_kernel<32,128,1,reparam,conv,trans,inj=0>",
                     "sigma_packed": "fused_fwd_kernel<32,128,1,reparam,conv,trans,inj=0>",
                     "out": "fused_fast_kernel<32,128,1,reparam,conv,notrans,inj=0,xmode=1,npw=8,pool=0>"},
             single_info={"mu_packed": (0, 0, 0, 0, 2, 1, 2), "sigma_packed": (0, 0, 0, 0, 2, 1, 2)}),
    "g_packs": _row(False, 'conv', (8, 32, 3, 1, 1, 8, 32), 1, ops=('mu_packed', 'sigma_packed'),
             aligned="fused_split_kernel<64,128,bf16x3,6 terms,npw=8,xm=0>", info=(0, 2, 8, 8, 16, 1, 16),
             together="fused_fwd_kernel<32,128,1,reparam,conv,trans,inj=0>", together_info=(0, 0, 0, 0, 16, 1, 16),
             single={"mu_packed": "fused_fwd_kernel<32,128,1,reparam,conv,trans,inj=0>",
                     "sigma_packed": "fused_fwd_kernel<32,128,1,reparam,conv,trans,inj=0>"},
             single_info={"mu_packed": (0, 0, 0, 0, 16, 1, 16), "sigma_packed": (0, 0, 0, 0, 16, 1, 16)}),
    "p_lin4": _row(False, 'linear', (64, 10, 0, 0, 0, 0, 8), 2, ops=('x', 'mu_w', 'rho_w'), mode=1,
             aligned="fused_fast_kernel<128,32,4,reparam,linear,trans,inj=0,xmode=0,npw=4,pool=0>", info=(0, 32, 1, 1, 1, 1, 2),
             together="fused_fast_kernel<128,32,4,reparam,conv,trans,inj=0,xmode=0,npw=8,pool=0>", together_info=(0, 32, 1, 1, 1, 1, 2),
             single={"x": "fused_fast_kernel<128,32,4,reparam,conv,trans,inj=0,xmode=0,npw=8,pool=0>",
                     "mu_w": "fused_fast_kernel<128,32,4,reparam,conv,trans,inj=0,xmode=2,npw=8,pool=0>",
                     "rho_w": "fused_fast_kernel<128,32,4,reparam,conv,trans,inj=0,xmode=2,npw=8,pool=0>"},
             single_info={}),
    "p_lin130": _row(False, 'linear', (130, 10, 0, 0, 0, 0, 8), 2, ops=('x', 'mu_w', 'rho_w'), mode=1,
             aligned="fused_fast_kernel<128,32,4,reparam,conv,trans,inj=0,xmode=0,npw=8,pool=0>", info=(0, 32, 1, 1, 1, 1, 2),
             together="fused_fast_kernel<128,32,4,reparam,conv,trans,inj=0,xmode=0,npw=8,pool=0>", together_info=(0, 32, 1, 1, 1, 1, 2),
             single={},
             single_info={}),
    "n_r": _row(False, 'conv', (8, 32, 3, 1, 1, 8, 4), 2, ops=('eps_w', 'eps_b'), nat=True, bias=True,
             aligned="fused_fwd_kernel<32,128,1,reparam,conv,trans,inj=1>", info=(0, 0, 0, 0, 2, 1, 4),
             together="fused_fwd_kernel<32,128,1,reparam,conv,trans,inj=1>", together_info=(0, 0, 0, 0, 2, 1, 4),
             single={"out": "fused_fwd_kernel<32,128,1,reparam,conv,notrans,inj=1>"},
             single_info={}),
    "n_f": _row(True, 'conv', (8, 32, 3, 1, 1, 8, 4), 2, ops=('sign_out', 'eps_w', 'sign_in'), nat=True,
             aligned="fused_fwd_kernel<32,128,1,flip,conv,trans,inj=1>", info=(0, 0, 0, 0, 2, 1, 4),
             together="fused_fwd_kernel<32,128,1,flip,conv,notrans,inj=1>", together_info=(0, 0, 0, 0, 2, 1, 4),
             single={"sign_out": "fused_fwd_kernel<32,128,1,flip,conv,notrans,inj=1>",
                     "out": "fused_fwd_kernel<32,128,1,flip,conv,notrans,inj=1>"},
             single_info={}),
    "n_lin": _row(True, 'linear', (64, 10, 0, 0, 0, 0, 8), 2, ops=('eps_w', 'sign_in', 'sign_out'), nat=True,
             aligned="fused_fwd_kernel<128,32,4,flip,linear,trans,inj=1>", info=(0, 0, 0, 0, 1, 1, 2),
             together="fused_fwd_kernel<128,32,4,flip,conv,trans,inj=1>", together_info=(0, 0, 0, 0, 1, 1, 2),
             single={"eps_w": "fused_fwd_kernel<128,32,4,flip,conv,trans,inj=1>",
                     "sign_in": "fused_fwd_kernel<128,32,4,flip,conv,trans,inj=1>"},
             single_info={}),
}


def geometry(row):
    """-> dict(B, Ci, H, W, Co, k, st, pad, Ho, Wo) of the row's launch (Linear as the 1 x 1 convolution of a 1 x 1 image)."""
    Ci, Co, k, st, pad, H, B = row["geo"]
    if row["kind"] == "linear":
        return dict(B=B, Ci=Ci, H=1, W=1, Co=Co, k=1, st=1, pad=0, Ho=1, Wo=1)
    Hv = H if row["kind"] != "updil" else (H - 1) * UPDIL[0] + 1 + UPDIL[2] + UPDIL[3]
    Ho = (Hv + 2 * pad - k) // st + 1
    return dict(B=B, Ci=Ci, H=H, W=H, Co=Co, k=k, st=st, pad=pad, Ho=Ho, Wo=Ho)


class Seam:
    """The C ABI in plan-only mode with made-up addresses, the way tools/record_fp32_plans.py drives it."""

    def __init__(self):
        from bayesian_torch_amd import _lib
        self.m, self.L = _lib, _lib.lib()
        self.h = C.CDLL(_lib.LIB_PATH)      # the bt_debug_* hooks are outside include/bt_hip.h
        self.info = (C.c_int64 * 16)()

    def plan(self, row, off=0, which=None):
        """The row's launch with the operands ``which`` (default: the row's ``ops``) at address + 4 * off
        -> (return code, kernel name or the refusal's text, launch info)."""
        m, L = self.m, self.L
        g = geometry(row)
        which = row["ops"] if which is None else which
        a = lambda name, present=True: (P + (4 * off if name in which else 0)) if present else None
        flip, bias, nat = row["flip"], row["bias"], row["nat"]
        par = m.bt_params(a("mu_w"), a("rho_w"), a("mu_b", bias), a("rho_b", bias), a("prior_mu_w", row["kl"]), a("prior_sigma_w", row["kl"]),
                          a("prior_mu_b", row["kl"] and bias), a("prior_sigma_b", row["kl"] and bias), a("mu_packed", row["packs"]),
                          a("sigma_packed", row["packs"]), 0, 0)
        draws = m.bt_draws(a("eps_w", nat), a("eps_b", nat and bias), a("sign_in", nat and flip), a("sign_out", nat and flip), m.bt_rng(1, None, 0, 1, 0, 0))
        x_elems = g["B"] * g["Ci"] * g["H"] * g["W"]
        out_elems = g["B"] * g["Co"] * g["Ho"] * g["Wo"]
        ep = None
        if row["res"] or row["pool"]:
            ep = m.bt_epilogue(a("post_scale", row["res"]), a("post_shift", row["res"]), a("residual", row["res"]), out_elems if row["res"] else 0,
                               1 if row["res"] else 0, 1 if row["pool"] else 0)
        geom = m.bt_conv2d_geom(g["B"], g["Ci"], g["H"], g["W"], g["Co"], g["k"], g["k"], g["st"], g["st"], g["pad"], g["pad"], 1, 1, 1)
        ws_bytes = m.WORKSPACE_BYTES + int(L.bt_fused_scratch_bytes(C.byref(geom), row["S"]))
        tail = (row["S"], a("x"), x_elems if row["stacked"] else 0, C.byref(par), C.byref(draws), None if ep is None else C.byref(ep), a("out"),
                P if row["kl"] else None, P, ws_bytes, None)
        before, spw = L.bt_get_contraction(), os.environ.get("BT_QUAD_SPW")
        os.environ["BT_QUAD_SPW"] = "1"     # the sample walk is planned from the device's CU count: a machine without one plans the one-sample path
        self.h.bt_debug_plan_only(1)
        try:
            assert L.bt_set_contraction(row["mode"]) == 0
            if row["kind"] == "linear":
                rc = (L.bt_flipout_linear_fwd if flip else L.bt_reparam_linear_fwd)(g["B"], g["Ci"], g["Co"], *tail)
            elif row["kind"] == "updil":
                u = m.bt_updil(*UPDIL)
                rc = (L.bt_flipout_conv2d_updil_fwd if flip else L.bt_reparam_conv2d_updil_fwd)(C.byref(geom), C.byref(u), *tail)
            else:
                rc = (L.bt_flipout_conv2d_fwd if flip else L.bt_reparam_conv2d_fwd)(C.byref(geom), *tail)
        finally:
            self.h.bt_debug_plan_only(0)
            L.bt_set_contraction(before)
            if spw is None:
                del os.environ["BT_QUAD_SPW"]
            else:
                os.environ["BT_QUAD_SPW"] = spw
        if rc != 0:
            return rc, L.bt_last_error_string().decode(), None
        L.bt_last_launch_info(self.info, 16)
        return rc, L.bt_last_kernel_name().decode(), dict(zip(m.LAUNCH_INFO_FIELDS, (int(v) for v in self.info)))
