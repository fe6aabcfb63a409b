"""Worker of tests/test_trainer_optimizer.py::test_two_ranks_accumulate_and_clip: started twice by `python -m torch.distributed.run` (gloo; both
ranks share the one GPU of the box), NOT collected by pytest.  Beside tests/two_rank_training_worker.py, for the optimizer options.

Every rank trains `ModifiedFPN` through `DepthCompletionTrainer(max_grad_norm=..., weight_decay=..., decoupled_weight_decay=True)`: two windows
of two micro-steps each, `backward_only(shard A of the rank); step(shard B of the rank)`.  Beside it one single-process trainer computes the
four shard gradients of a window (both ranks' A and B) with `forward_backward` and adds them up itself:

    g_sum = (g(B, rank 0) + g(A, rank 0)) + (g(B, rank 1) + g(A, rank 1))      fp32; each sum has two terms: the order cannot matter

The distributed trainer's flat gradient after the step must equal g_sum bit for bit (the window's sum was added BEFORE the one all-reduce: the
closing step takes the uncut path), `last_grad_norm` must be the float64 norm of g_sum and equal on both ranks, and so must the checksum of
flat_p.  The single-process trainer then takes the same update, so that the second window starts from the same weights."""
import os
import sys

import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    assert world == 2
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    dist.init_process_group("gloo")
    from vi_depth_completion_amd import synthetic as S
    from vi_depth_completion_amd.networks.depth_completion import ModifiedFPN
    from vi_depth_completion_amd.training import DepthCompletionTrainer
    B, H, W = 2, 64, 96

    def shard(seed):
        g = torch.Generator().manual_seed(seed)
        img = torch.rand(B, 3, H, W, generator=g)
        nrm = torch.nn.functional.normalize(torch.randn(B, 3, H, W, generator=g), dim=1)
        dep = torch.rand(B, 1, H, W, generator=g) * (torch.rand(B, 1, H, W, generator=g) < 0.02)
        gt = torch.rand(B, 1, H, W, generator=g) * 4 + 0.5
        return [t.to(dev) for t in (img, nrm, dep, gt)]

    def model():
        m = ModifiedFPN().to(dev)
        m.load_state_dict(S.seeded_state_dict(m.state_dict(), 7, device=dev))
        m.train()
        return m

    options = dict(weight_decay=0.05, decoupled_weight_decay=True)
    t_dist = DepthCompletionTrainer(model(), 1e-4, max_grad_norm=1.0, **options)
    assert t_dist._distributed() and t_dist.layout == "grouped"
    single = DepthCompletionTrainer(model(), 1e-4, max_grad_norm=1.0, **options)      # the same layout (built under the process group), no collectives
    single._distributed = lambda: False
    single.buckets.all_reduce_async = lambda *a, **k: []
    norms = []
    for window in range(2):
        shards = {(r, s): shard(100 + 10 * window + 2 * r + s) for r in range(2) for s in range(2)}      # (rank, micro-step)
        loss_a = t_dist.backward_only(*shards[rank, 0])
        assert t_dist._window == 1 and t_dist.step_count == window
        loss_b = t_dist.step(*shards[rank, 1])
        g, losses = {}, {}
        for key, ins in shards.items():
            losses[key] = single.forward_backward(*ins)[0]
            g[key] = single.flat_g.clone()
        assert float(loss_a) == float(losses[rank, 0]) and float(loss_b) == float(losses[rank, 1]), (window, float(loss_a), float(loss_b))
        want = (g[0, 1] + g[0, 0]) + (g[1, 1] + g[1, 0])
        if not torch.equal(t_dist.flat_g, want):
            d = (t_dist.flat_g - want).abs()
            raise AssertionError("window %d: the all-reduced gradient differs from the sum of the four shard gradients: %d elements, max %.3e (scale %.3e)"
                                 % (window, int((d > 0).sum()), float(d.max()), float(want.abs().max())))
        n = want.numel()
        norm64 = float(torch.sqrt((want.double() ** 2).sum()))
        norm = float(t_dist.last_grad_norm)
        assert abs(norm - norm64) <= n * 2.0 ** -52 * norm64, (window, norm, norm64)
        single.flat_g.copy_(want)
        single.optimizer_step(reduced=True)
        assert torch.equal(single.flat_p, t_dist.flat_p), "window %d: the update differs from the single-process trainer's on the same gradient" % window
        mine = torch.stack([t_dist.last_grad_norm.cpu(), t_dist.flat_p.double().sum().cpu()])
        both = [torch.zeros_like(mine) for _ in range(2)]
        dist.all_gather(both, mine)
        assert torch.equal(both[0], both[1]), (window, both)
        norms.append(norm)
    assert norms[0] > 1.0, "max_grad_norm = 1 must bite: %r" % norms
    torch.cuda.synchronize()
    dist.barrier()
    dist.destroy_process_group()
    if rank == 0:
        print("TWO_RANK_OPTIMIZER_OK norms=%s" % [round(x, 6) for x in norms])


if __name__ == "__main__":
    main()
