"""Launched by tests/test_gpu_optim.py under torch.distributed.run with 2 ranks on ONE GPU with backend
gloo (the rehearsal a one-GPU box allows, as scripts/ddp_check.py): gradient clipping in a multi-rank
Trainer.  The norm the guarded Adam step clips by must be that of the AVERAGED gradient (both launches
sit after the all-reduce), so every rank takes the same clip factor and the ranks stay identical.  The
eager run probes the gradient vector around the all-reduce; a second run replays the step from graphs."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "point-cloud-audio_amd")]
import numpy as np, torch, torch.distributed as dist
import dataset, models
from pca_hip import _lib, trainer


class Probe(trainer.Trainer):
    """Eager steps only: the float64 norm of this rank's own gradient (after the backward) and of the
    averaged one (after the all-reduce, as Adam is about to see it), and what the step then reports."""
    local_norms = avg_norms = reported = None

    def _seg0(self):
        super()._seg0()
        if self.local_norms is not None:
            self.local_norms.append(float(self.eng.grads.double().norm()))

    def _seg2(self):
        if self.avg_norms is not None:
            self.avg_norms.append(float((self.eng.grads.double() / self.world).norm()))
        super()._seg2()
        if self.reported is not None:
            self.reported.append(self.read_optim_stats(reset=False)["last_grad_norm"])


def build(pg, use_graph, probe, **options):
    rng = np.random.Generator(np.random.PCG64(5))
    F, Tn, Cc, B = 64, 320, 10, 16
    x = rng.normal(-9, 3, size=(F, Tn)).astype(np.float32)
    y = rng.integers(0, Cc, size=(Tn,))
    torch.manual_seed(3)
    net = models.ST(dim_input=2, dim_output=Cc, num_inds=16, dim_hidden=128, num_heads=4).to(dev)
    ds = dataset.ESC_pc(x, y, np.linspace(0, 0.5, F), device=dev)
    tr = Probe(net, ds, B, mode=_lib.MODE_F32, use_graph=use_graph, seed=11, shuffle=True,
               process_group=pg, overlap=False, **options)
    if probe:
        tr.local_norms, tr.avg_norms, tr.reported = [], [], []
    return tr


def ranks_identical(flat):
    gathered = [torch.zeros_like(flat) for _ in range(world)]
    dist.all_gather(gathered, flat)
    return all(torch.equal(gathered[0], g) for g in gathered)


if __name__ == "__main__":
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    dist.init_process_group("gloo")
    pg = dist.group.WORLD
    # one unclipped step to find the scale: M = half the averaged gradient's norm, rank 0's word
    tr = build(pg, False, True, skip_nonfinite=True)
    tr.step()
    M = torch.tensor([0.5 * tr.avg_norms[0]], dtype=torch.float64)
    dist.broadcast(M, src=0)
    M = float(M)

    tr = build(pg, False, True, max_grad_norm=M)
    for _ in range(4):
        tr.step()
    torch.cuda.synchronize()
    stats = tr.read_optim_stats()
    flat = tr.eng.flat.detach().cpu().clone()
    same = ranks_identical(flat)
    mine = torch.tensor(tr.local_norms, dtype=torch.float64)
    both = [torch.zeros_like(mine) for _ in range(world)]
    dist.all_gather(both, mine)
    differ = bool(((both[0] - both[1]).abs() > 1e-3 * both[0]).all())
    rep, avg = np.array(tr.reported), np.array(tr.avg_norms)
    # at most 17 fp32 terms in a thread's sum at this size (8.5 * 2^-24 on the norm) and the fp32
    # rounding of the result (2^-24): 5.7e-7 in all
    of_average = bool(np.all(np.abs(rep - avg) <= 2e-6 * avg))
    not_local = bool(np.all(np.abs(rep - mine.numpy()) > 1e-3 * avg))

    trg = build(pg, True, False, max_grad_norm=M)
    for _ in range(4):
        trg.step()
    torch.cuda.synchronize()
    gsame = ranks_identical(trg.eng.flat.detach().cpu().clone())
    gstats = trg.read_optim_stats()
    if rank == 0:
        print("M", M, "local", both[0].tolist(), both[1].tolist(), "averaged", avg.tolist(),
              "reported", rep.tolist(), flush=True)
        print("RANKS_IDENTICAL", same)
        print("LOCAL_NORMS_DIFFER", differ)
        print("NORM_IS_OF_THE_AVERAGE", of_average)
        print("NORM_IS_NOT_LOCAL", not_local)
        print("CLIPPED", stats["clipped"], "of 4; under graphs", gstats["clipped"])
        print("GRAPH_RANKS_IDENTICAL", gsame, flush=True)
    dist.barrier()
    dist.destroy_process_group()
