"""What the low-rank layer's training tests share (a plain module, imported the way _lowrank_ref.py is): the closed-form gradient of the
KL in float64 torch ops, and the float64 autograd reference of one training loss on given draws."""
import torch

import _lowrank_ref as R


def kl_grad_closed_form(mu, L, D, prior_mean, prior_var, c=1.0):
    """(dKL/dmu, dKL/dL) * c of KL( N(mu, L L^T + d I) || N(m, diag P) ), un-normalised, d = D[0] (a constant diagonal):
        dmu = c (mu - m) / P,      dL = c (L / P - L (d I + L^T L)^-1)      (row i of L over P_i).
    No autograd. (d I + L^T L)^-1 = (1 / d) G^-1 with G = I + L^T L / d, the matrix the forward factorises; it is applied by a linear
    solve in double, in that scaled form: forming d I + L^T L first adds 1e-10 to entries of order one and costs a digit."""
    mu, L, D, m, P = (t.detach().double() for t in (mu, L, D, prior_mean, prior_var))
    d = D.reshape(-1)[0]
    assert bool((D == d).all()), "the closed form is for a constant diagonal"
    r = L.shape[1]
    G = torch.eye(r, dtype=torch.float64) + L.t() @ (L / d)
    return c * (mu - m) / P, c * (L / P[:, None] - torch.linalg.solve(G, (L / d).t()).t())      # (G is symmetric: (L / d) G^-1 = (G^-1 (L / d)^T)^T)


def reference(g, x, z, eps, gy, shared=True, kl_weight=1.0, normalised=True):
    """fp64 autograd of  (out * gy).sum() + kl_weight * KL [/ n]  for the golden ``g`` on the draws (z [S, r], eps [S, n]), x as given
    -> dict(out, kl, dx, dmu, dL), all double CPU tensors."""
    xr = x.detach().cpu().double().requires_grad_(True)
    mur, Lr = g["mu_kernel"].double().requires_grad_(True), g["L_param"].double().requires_grad_(True)
    out = R.forward(xr, mur, Lr, g["D_param"], z.detach().cpu(), eps.detach().cpu(), g["meta"]["ctor"], shared)
    kl = R.kl_diag(mur, Lr, g["D_param"], g["prior_mean"], g["prior_cov_D"])
    if normalised:
        kl = kl / mur.numel()
    ((out * gy.detach().cpu().double()).sum() + kl_weight * kl).backward()
    return dict(out=out.detach(), kl=kl.detach(), dx=xr.grad, dmu=mur.grad, dL=Lr.grad)
