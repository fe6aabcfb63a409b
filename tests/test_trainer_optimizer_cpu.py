"""CPU: the float64 restatement of the trainers' optimizer options (tests/optim_ref.py) against torch's own optimizers and clip_grad_norm_ run in
float64, and the segment-table builder of training.py on fake parameter lists in both flat orders."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import optim_ref as R                                                    # noqa: E402
from vi_depth_completion_amd.training import build_segment_table        # noqa: E402

TABLE = ([0, 5, 6, 40, 57], [1.0, 0.5, 2.0, 1.0], [0.0, 0.1, 0.01, 0.3], [0, 0, 1, 0])      # a 1-element segment, a frozen one


@pytest.mark.parametrize("decoupled", [False, True])
@pytest.mark.parametrize("table", [None, ([0, 57], [1.0], [0.05], [0]), TABLE], ids=["plain", "decay", "groups"])
@pytest.mark.parametrize("max_norm", [None, 0.5, 1e9])
def test_restatement_equals_torch_in_float64(decoupled, table, max_norm):
    """Three steps of torch.optim.Adam(weight_decay) / torch.optim.AdamW (one param group per segment, frozen segments outside the optimizer)
    behind torch.nn.utils.clip_grad_norm_, all in float64 on the CPU, against optim_ref: parameters, norms and clip factors to 1e-12 relative."""
    rng = np.random.default_rng(5)
    n, lr = 57, 1e-2
    p0 = rng.standard_normal(n)
    grads = [rng.standard_normal(n) * 10.0 ** (s - 3) for s in (1, 2, 3)]
    begin, scale, decay, flags = table if table is not None else ([0, n], [1.0], [0.0], [0])
    parts = [torch.tensor(p0[begin[i]:begin[i + 1]], dtype=torch.float64).requires_grad_(True) for i in range(len(scale))]
    live = [i for i in range(len(scale)) if not flags[i] & 1]
    opt = (torch.optim.AdamW if decoupled else torch.optim.Adam)([{"params": [parts[i]], "lr": lr * scale[i], "weight_decay": decay[i]} for i in live], lr=lr)
    p, m, v = p0.copy(), np.zeros(n), np.zeros(n)
    frozen = R.expand_segments(n, table)[2]
    for step, g in enumerate(grads, 1):
        for i, q in enumerate(parts):
            q.grad = torch.tensor(g[begin[i]:begin[i + 1]], dtype=torch.float64)
        norm, factor = R.norm_and_factor(g, frozen, 1.0, max_norm)
        if max_norm is not None:
            total = torch.nn.utils.clip_grad_norm_([parts[i] for i in live], max_norm)
            assert abs(float(total) - norm) <= 1e-12 * norm
            clipped = np.concatenate([parts[i].grad.numpy() for i in live])
            assert np.abs(clipped - (g * factor)[~frozen]).max() <= 1e-12 * np.abs(clipped).max()
            assert (factor < 1.0) == (norm > max_norm)
        opt.step()
        p, m, v = R.optimizer_step(p, g, m, v, step, lr, factor=factor, decoupled=decoupled, table=table)
    want = torch.cat([q.detach() for q in parts]).numpy()
    assert np.abs(p - want).max() <= 1e-12 * np.abs(want).max()
    assert np.array_equal(p[frozen], p0[frozen]) and not np.any(p[~frozen] == p0[~frozen])
    # (the helper the GPU tests measure torch's fp32 error with runs the same optimizers)
    factors = [R.norm_and_factor(g, frozen, 1.0, max_norm)[1] for g in grads]
    assert np.abs(R.torch_steps(p0, grads, lr, torch.float64, decoupled, table, factors) - want).max() <= 1e-12 * np.abs(want).max()


def test_norm_scale_and_mean_of_a_window():
    """grad_scale = 1 / k: the norm and the factor are those of the mean gradient."""
    g = np.random.default_rng(1).standard_normal(100)
    norm, factor = R.norm_and_factor(g, None, 0.25, 0.1)
    n4, f4 = R.norm_and_factor(g / 4, None, 1.0, 0.1)
    assert abs(norm - n4) <= 1e-15 * n4 and abs(factor - 0.25 * f4) <= 1e-15 * factor
    assert R.norm_and_factor(g, None, 0.25, None) == (norm, 0.25)


def _flat(layout):
    """A fake `named` list (name, numel) in the trainer's two orders: three pyramids with the same four tensors, then a decoder."""
    pyr, tensors = ("resnet_rgb", "resnet_normal", "resnet_depth"), [("conv1.weight", 27), ("bn1.weight", 1), ("bn1.bias", 1), ("layer1.0.conv.weight", 64)]
    dec = [("feature1.0.weight", 30), ("feature1.0.bias", 1), ("feature_concat.2.weight", 7)]
    if layout == "grouped":
        return [(p + "." + k, n) for k, n in tensors for p in pyr] + dec
    return [(p + "." + k, n) for p in pyr for k, n in tensors] + dec


@pytest.mark.parametrize("layout", ["per_pyramid", "grouped"])
def test_segment_table_builder(layout):
    named = _flat(layout)
    total = sum(n for _, n in named)
    offs, o = {}, 0
    for k, n in named:
        offs[k] = (o, o + n)
        o += n

    def settings_of(table, name):
        begin, scale, decay, flags = table
        a, b = offs[name]
        s = [i for i in range(len(scale)) if begin[i] <= a and b <= begin[i + 1]]
        assert len(s) == 1, "a tensor lies inside exactly one segment"
        return scale[s[0]], decay[s[0]], flags[s[0]]

    def covers(table):
        begin = table[0]
        assert begin[0] == 0 and begin[-1] == total and all(a < b for a, b in zip(begin[:-1], begin[1:]))
        assert len(begin) == len(table[1]) + 1 == len(table[2]) + 1 == len(table[3]) + 1
        assert all((table[1][i], table[2][i], table[3][i]) != (table[1][i + 1], table[2][i + 1], table[3][i + 1]) for i in range(len(table[1]) - 1)), "equal neighbours merge"

    # no groups: one segment at the constructor's decay
    t = build_segment_table(named, None, 0.0)
    assert t == ([0, total], [1.0], [0.0], [0])
    assert build_segment_table(named, [], 0.25) == ([0, total], [1.0], [0.25], [0])
    # one pyramid by prefix: contiguous per pyramid (3 segments: before / it / after), interleaved per name when grouped
    t = build_segment_table(named, [("resnet_normal.", {"lr_scale": 0.1, "weight_decay": 0.5})], 0.01)
    covers(t)
    assert len(t[1]) == (3 if layout == "per_pyramid" else 9)
    for k, _ in named:
        assert settings_of(t, k) == ((0.1, 0.5, 0) if k.startswith("resnet_normal.") else (1.0, 0.01, 0)), k
    # first match wins; a callable; a 1-element tensor of its own; frozen; an option left out takes the constructor's value
    groups = [(lambda k: k.endswith("bn1.bias"), {"weight_decay": 0.0}), ("resnet_rgb.bn1", {"frozen": True}), ("resnet_", {"lr_scale": 2.0}),
              ("resnet_rgb.", {"lr_scale": 7.0})]
    t = build_segment_table(named, groups, 0.3)
    covers(t)
    assert settings_of(t, "resnet_rgb.bn1.bias") == (1.0, 0.0, 0)            # the callable comes first
    assert settings_of(t, "resnet_rgb.bn1.weight") == (1.0, 0.3, 1)          # frozen, 1 element
    assert settings_of(t, "resnet_rgb.conv1.weight") == (2.0, 0.3, 0)        # "resnet_" before "resnet_rgb."
    assert settings_of(t, "feature1.0.bias") == (1.0, 0.3, 0)
    a, b = offs["resnet_rgb.bn1.weight"]
    assert b - a == 1 and a in t[0] and b in t[0]
    # neighbours with equal settings merge across tensor names: the decoder is one segment
    t = build_segment_table(named, [("feature", {"frozen": True})], 0.0)
    covers(t)
    assert t == ([0, offs["feature1.0.weight"][0], total], [1.0, 1.0], [0.0, 0.0], [0, 1])
    with pytest.raises(ValueError):
        build_segment_table(named, [("feature", {"lr": 0.1})])
