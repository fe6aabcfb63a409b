"""float64 numpy restatement of the trainers' optimizer options (csrc/optim.hip): the Adam step with weight decay in torch.optim.Adam's L2 form
or torch.optim.AdamW's decoupled form, per-element learning-rate scales / decays / frozen flags expanded from a segment table, and the total
norm and clip factor of torch.nn.utils.clip_grad_norm_.  tests/test_trainer_optimizer_cpu.py pins it against torch's own optimizers run in
float64; tests/test_trainer_optimizer.py measures the kernels against it.  Not collected by pytest."""
import numpy as np


def expand_segments(n, table=None):
    """(lr_scale, weight_decay, frozen) per element from a table (begin, lr_scale, weight_decay, flags); None: scale 1, decay 0, not frozen."""
    scale, decay, frozen = np.ones(n), np.zeros(n), np.zeros(n, bool)
    if table is not None:
        begin, s, w, f = table
        assert begin[0] == 0 and begin[-1] == n and all(a < b for a, b in zip(begin[:-1], begin[1:]))
        for i in range(len(s)):
            scale[begin[i]:begin[i + 1]], decay[begin[i]:begin[i + 1]], frozen[begin[i]:begin[i + 1]] = s[i], w[i], bool(f[i] & 1)
    return scale, decay, frozen


def norm_and_factor(g, frozen=None, grad_scale=1.0, max_norm=None):
    """clip_grad_norm_ on grad_scale * g over the non-frozen elements: (total norm, the factor the optimizer multiplies g by)."""
    g = np.asarray(g, np.float64)
    if frozen is not None:
        g = g[~frozen]
    norm = grad_scale * np.sqrt(np.sum(g * g))
    if max_norm is None or not max_norm > 0:
        return norm, grad_scale
    return norm, grad_scale * min(1.0, max_norm / (norm + 1e-6))


def optimizer_step(p, g, m, v, step, lr, betas=(0.9, 0.999), eps=1e-8, factor=1.0, decoupled=False, table=None):
    """One step (step = 1, 2, ...) on float64 copies; returns the new (p, m, v).  `factor` multiplies the gradient (norm_and_factor)."""
    p, g, m, v = (np.array(a, np.float64) for a in (p, g, m, v))
    scale, decay, frozen = expand_segments(p.size, table)
    b1, b2 = betas
    lr_e = lr * scale
    ge = g * factor
    p_in = p.copy()
    if decoupled:
        p = p * (1.0 - lr_e * decay)
    else:
        ge = ge + decay * p
    m_new = m * b1 + ge * (1.0 - b1)
    v_new = v * b2 + ge * ge * (1.0 - b2)
    denom = np.sqrt(v_new) / np.sqrt(1.0 - b2 ** step) + eps
    p_new = p - (lr_e / (1.0 - b1 ** step)) * (m_new / denom)
    return np.where(frozen, p_in, p_new), np.where(frozen, m, m_new), np.where(frozen, v, v_new)


def torch_steps(p0, grads, lr, dtype, decoupled=False, table=None, factors=None, betas=(0.9, 0.999), eps=1e-8):
    """torch's own CPU optimizer in `dtype` over the gradients `grads` (one per step): torch.optim.Adam(weight_decay=...) or torch.optim.AdamW
    with one parameter group per segment (lr = lr * lr_scale), frozen segments outside the optimizer; `factors`: per step, the factor the
    gradient is multiplied by first (in `dtype`).  Returns the stepped parameters (numpy, dtype)."""
    import torch
    n = len(p0)
    begin, scale, decay, flags = table if table is not None else ([0, n], [1.0], [0.0], [0])
    parts = [torch.tensor(np.asarray(p0[begin[i]:begin[i + 1]]), dtype=dtype).requires_grad_(True) for i in range(len(scale))]
    groups = [{"params": [parts[i]], "lr": lr * scale[i], "weight_decay": decay[i]} for i in range(len(scale)) if not flags[i] & 1]
    opt = (torch.optim.AdamW if decoupled else torch.optim.Adam)(groups, lr=lr, betas=betas, eps=eps) if groups else None
    for it, g in enumerate(grads):
        gt = torch.tensor(np.asarray(g), dtype=dtype)
        if factors is not None:
            gt = gt * torch.tensor(factors[it], dtype=dtype)
        for i, q in enumerate(parts):
            q.grad = gt[begin[i]:begin[i + 1]].clone()
        if opt is not None:
            opt.step()
    return torch.cat([q.detach() for q in parts]).numpy()
