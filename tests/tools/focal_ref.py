"""The specification of the focal cross entropy (fu_loss_ce_focal): torch on the CPU, fp64, written with log_softmax; the
gradient comes by autograd.  Over the valid pixels (target != ignore_index, 0 <= target < C), with p = softmax(z), q = p[t],
u = 1 - q, w the class weights (all ones when absent) and gamma >= 0:

    loss = sum_i w[t_i] * u_i^gamma * (-log q_i) / D,    D = sum_i w[t_i]

and loss 0 where D == 0 (the project's rule for the all-ignored batch).  gamma = 0 is
torch.nn.functional.cross_entropy(weight=, ignore_index=)."""
import torch
import torch.nn.functional as F


def _valid(target, ignore_index, C):
    return (target != ignore_index) & (target >= 0) & (target < C)


def focal_loss(logits, target, gamma, weight=None, ignore_index=-100):
    """logits: [B, C, H, W] (any float dtype, computed in fp64; autograd flows when it is an fp64 leaf); target: int64
    [B, H, W]; weight: None or C numbers, rounded to fp32 first as the kernel sees them.  Returns the fp64 scalar loss."""
    z = logits if logits.dtype == torch.float64 else logits.double()
    C = z.shape[1]
    w = torch.ones(C, dtype=torch.float64) if weight is None else torch.as_tensor(weight, dtype=torch.float32).double()
    valid = _valid(target, ignore_index, C)
    t = torch.where(valid, target, torch.zeros_like(target))
    logq = F.log_softmax(z, dim=1).gather(1, t.unsqueeze(1)).squeeze(1)          # [B, H, W]
    u = -torch.expm1(logq)                                                       # 1 - q without the cancellation
    wt = w[t] * valid
    D = wt.sum()
    if float(D) == 0.0:
        return z.sum() * 0.0
    # 0^0 = 1 (gamma = 0); where u == 0 and gamma > 0 the term is 0 and so is its gradient (clamp: no 0^(gamma-1) in autograd)
    mod = torch.ones_like(u) if gamma == 0 else torch.where(u > 0, u.clamp_min(1e-300) ** gamma, torch.zeros_like(u))
    return (wt * mod * (-logq)).sum() / D


def focal_dlogits_closed_form(logits, target, gamma, weight=None, ignore_index=-100):
    """dL/dz_k = w[t] (p_k - [k == t]) m / D,  m = u^gamma - gamma q u^(gamma-1) log q,  fp64 [B, C, H, W]."""
    z = logits.detach().double()
    C = z.shape[1]
    w = torch.ones(C, dtype=torch.float64) if weight is None else torch.as_tensor(weight, dtype=torch.float32).double()
    valid = _valid(target, ignore_index, C)
    t = torch.where(valid, target, torch.zeros_like(target))
    logp = F.log_softmax(z, dim=1)
    p = logp.exp()
    logq = logp.gather(1, t.unsqueeze(1)).squeeze(1)
    q, u = logq.exp(), -torch.expm1(logq)
    wt = w[t] * valid
    D = wt.sum()
    if float(D) == 0.0:
        return torch.zeros_like(z)
    if gamma == 0:
        m = torch.ones_like(u)
    else:
        m = torch.where(u > 0, u ** gamma - gamma * q * u.clamp_min(1e-300) ** (gamma - 1) * logq, torch.zeros_like(u))
    onehot = F.one_hot(t, C).permute(0, 3, 1, 2).double()
    return (wt * m / D).unsqueeze(1) * (p - onehot)
