"""The specification of the decoupled weight decay inside the fused Adam step (fu_set_weight_decay): torch.optim.AdamW's
single-tensor path on float32, restated.  For one tensor, with the step's lr and t the 1-based step count:

    if the tensor decays:   p = p * float32(1 - lr * weight_decay)        the factor formed in double, rounded once;
                                                                           one fp32 multiply (param.mul_)
    g      = g * float32(grad_scale)                                       (only when grad_scale != 1)
    m      = m.lerp_(g, 1 - beta1)
    v      = v.mul_(beta2).addcmul_(g, g, value=1 - beta2)
    denom  = (v.sqrt() / sqrt(1 - beta2^t)).add_(eps)
    p      = p.addcdiv_(m, denom, value=-lr / (1 - beta1^t))

The decay is a numpy float32 multiply; the Adam sequence is written with ATen's CPU tensor operations, which round every
operation on its own -- the sequence fu_adam_step restates on the device.  The moments never see the decay.
tests/test_weight_decay_cpu.py pins this file bit for bit against torch.optim.AdamW(foreach=False)."""
import numpy as np
import torch


def decay_factor(lr, weight_decay) -> np.float32:
    """float32(1 - lr * weight_decay): exactly 1 for weight_decay = 0."""
    return np.float32(1.0 - float(lr) * float(weight_decay))


def step_tensor(p, g, m, v, lr, betas, eps, t, weight_decay, decays, grad_scale=1.0):
    """One update of one tensor, in place on the CPU float32 tensors p, m, v; g is only read."""
    beta1, beta2 = betas
    if decays:
        p.copy_(torch.from_numpy(p.numpy() * decay_factor(lr, weight_decay)))
    if grad_scale != 1.0:
        g = g * float(np.float32(grad_scale))
    bc1 = 1 - beta1 ** t
    bc2 = 1 - beta2 ** t
    m.lerp_(g, 1 - beta1)
    v.mul_(beta2).addcmul_(g, g, value=1 - beta2)
    denom = (v.sqrt() / (bc2 ** 0.5)).add_(eps)
    p.addcdiv_(m, denom, value=-(lr / bc1))


def step_flat(p, g, m, v, table, flags, lr, betas, eps, t, weight_decay, grad_scale=1.0):
    """One update of flat CPU float32 buffers: table = [(offset, numel)] in parameter order, flags[k] = tensor k decays."""
    for (off, n), f in zip(table, flags):
        step_tensor(p[off:off + n], g[off:off + n], m[off:off + n], v[off:off + n], lr, betas, eps, t, weight_decay, bool(f),
                    grad_scale)


def max_abs_diff(a, b) -> float:
    return float((a.double() - b.double()).abs().max()) if a.numel() else 0.0
