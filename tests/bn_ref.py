"""Test infrastructure: train-mode BatchNorm + activation restated in plain float64 torch, from the formulas in the header of
csrc/batchnorm.hip (not from F.batch_norm: tests/test_batchnorm_ref_cpu.py pins the two to each other).

  x [B, C, N], statistics over (B, N) per channel, n = B * N
  mean = sum x / n                     var = sum (x - mean)^2 / n          (biased)
  invstd = 1 / sqrt(var + eps)         xhat = (x - mean) * invstd
  z = xhat * gamma + beta              out = act(z)                        act: 0 none | 1 SiLU | 2 ReLU
  running' = (1 - momentum) * running + momentum * (mean | var * n / (n - 1))        (the biased var when n == 1)
  dz = dy * act'(z)                    s1 = sum dz        s2 = sum dz * xhat         (grad beta, grad gamma)
  dx = (dz - s1 / count - xhat * s2 / count) * invstd * gamma   (train)    dx = dz * invstd * gamma   (eval)
  merge of ranks r with (mean_r, var_r, n_r):  n = sum n_r,  mean = sum n_r mean_r / n,
                                               var = sum n_r (var_r + (mean_r - mean)^2) / n

Inputs are fp32 (or any) tensors; everything is converted to float64 inside and returned as float64.

`flaw` plants ONE named error (FLAWS); it exists for the sensitivity checks of tests/test_batchnorm_ref_cpu.py, which show that
the bounds of tests/test_batchnorm_gpu.py are tight enough to tell a subtly wrong kernel from a right one.
"""
import torch

ACT_NONE, ACT_SILU, ACT_RELU = 0, 1, 2

FLAWS = ("biased_running_var",      # running_var takes the biased variance
         "dx_without_s2_term",      # the xhat * s2 / n term dropped from dx
         "s1_s2_swapped",           # the two backward sums exchanged
         "eps_outside_sqrt",        # invstd = 1 / (sqrt(var) + eps)
         "silu_grad_without_z_term",  # SiLU' = s instead of s * (1 + z * (1 - s))
         "merge_without_d2")        # the merged variance averages the ranks' variances without (mean_r - mean)^2


def _d(t):
    return None if t is None else torch.as_tensor(t).detach().to("cpu", torch.float64)


def _per_channel(v, C, fill):
    return torch.full((C,), fill, dtype=torch.float64) if v is None else _d(v).reshape(C)


def _invstd(var, eps, flaw):
    if flaw == "eps_outside_sqrt":
        return 1.0 / (var.sqrt() + eps)
    return 1.0 / (var + eps).sqrt()


def act_fwd(z, act):
    if act == ACT_SILU:
        return z * torch.sigmoid(z)
    if act == ACT_RELU:
        return z.clamp_min(0.0)
    assert act == ACT_NONE
    return z


def act_grad(z, act, flaw=None):
    if act == ACT_SILU:
        s = torch.sigmoid(z)
        return s if flaw == "silu_grad_without_z_term" else s * (1.0 + z * (1.0 - s))
    if act == ACT_RELU:
        return (z > 0).to(z.dtype)          # 0 at z == 0, as the kernels and the framework have it
    assert act == ACT_NONE
    return torch.ones_like(z)


def batch_stats(x):
    """x [B, C, N] -> mean [C], biased var [C] (two passes in float64)"""
    x = _d(x)
    mean = x.mean(dim=(0, 2))
    var = ((x - mean.view(1, -1, 1)) ** 2).mean(dim=(0, 2))
    return mean, var


def running_update(mean, var, count, momentum, running, flaw=None):
    """-> (running_mean', running_var'): the variance enters unbiased (biased when count == 1)"""
    rm, rv = _d(running[0]), _d(running[1])
    unb = var * (count / (count - 1.0)) if count > 1 and flaw != "biased_running_var" else var
    return (1.0 - momentum) * rm + momentum * mean, (1.0 - momentum) * rv + momentum * unb


def bn_act_fwd(x, gamma, beta, eps, act, mean=None, var=None, momentum=None, running=None, flaw=None):
    """-> out [B, C, N], mean [C], biased var [C], (running_mean', running_var') or None.
    mean / var given: they are used as they are (eval mode, or statistics merged across ranks)."""
    x = _d(x)
    B, C, N = x.shape
    if mean is None:
        mean, var = batch_stats(x)
    else:
        mean, var = _d(mean), _d(var)
    g, b = _per_channel(gamma, C, 1.0), _per_channel(beta, C, 0.0)
    xhat = (x - mean.view(1, C, 1)) * _invstd(var, eps, flaw).view(1, C, 1)
    out = act_fwd(xhat * g.view(1, C, 1) + b.view(1, C, 1), act)
    new_running = None if running is None else running_update(mean, var, B * N, momentum, running, flaw)
    return out, mean, var, new_running


def bn_act_bwd(x, dy, mean, var, gamma, beta, eps, act, train, count, flaw=None):
    """-> dx [B, C, N], s1 [C], s2 [C]"""
    x, dy, mean, var = _d(x), _d(dy), _d(mean), _d(var)
    B, C, N = x.shape
    g, b = _per_channel(gamma, C, 1.0), _per_channel(beta, C, 0.0)
    invstd = _invstd(var, eps, flaw).view(1, C, 1)
    xhat = (x - mean.view(1, C, 1)) * invstd
    dz = dy * act_grad(xhat * g.view(1, C, 1) + b.view(1, C, 1), act, flaw)
    s1, s2 = dz.sum(dim=(0, 2)), (dz * xhat).sum(dim=(0, 2))
    if flaw == "s1_s2_swapped":
        s1, s2 = s2, s1
    if train:
        t2 = 0.0 if flaw == "dx_without_s2_term" else xhat * (s2 / count).view(1, C, 1)
        dx = (dz - (s1 / count).view(1, C, 1) - t2) * invstd * g.view(1, C, 1)
    else:
        dx = dz * invstd * g.view(1, C, 1)
    return dx, s1, s2


def sync_merge(records, momentum=None, running=None, flaw=None):
    """records: one (mean [C], var [C], count) per rank -> mean, var, (running_mean', running_var') or None, 1 / n"""
    n = float(sum(float(r[2]) for r in records))
    mean = sum(_d(r[0]) * float(r[2]) for r in records) / n
    if flaw == "merge_without_d2":
        var = sum(_d(r[1]) * float(r[2]) for r in records) / n
    else:
        var = sum((_d(r[1]) + (_d(r[0]) - mean) ** 2) * float(r[2]) for r in records) / n
    new_running = None if running is None else running_update(mean, var, n, momentum, running)
    return mean, var, new_running, 1.0 / n
