"""Launched by tests/test_gpu_trainer_eval.py under torch.distributed.run with 2 ranks on ONE GPU with
backend gloo (the rehearsal a one-GPU box allows, as scripts/ddp_check.py): every rank builds the same
model and held-out set, trainer.Evaluator scores its contiguous shard, the counters, the confusion matrix
and the loss are all-reduced, and rank 0 writes what ``run()`` returned to $PCA_OUT.  The test compares
it with a single-rank pass over the whole set."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "point-cloud-audio_amd")]
import numpy as np, torch, torch.distributed as dist
import dataset, models
from pca_hip import _lib, trainer


def held_out(dev):
    """The model and held-out set of the sharding test: 333 sets (odd: the shards differ in size, and
    neither is a multiple of the batch), 10 classes."""
    rng = np.random.Generator(np.random.PCG64(17))
    F, T, C = 64, 333, 10
    x = rng.normal(-9, 3, size=(F, T)).astype(np.float32)
    y = rng.integers(0, C, size=(T,))
    torch.manual_seed(5)
    net = models.ST(dim_input=2, dim_output=C, num_inds=16, dim_hidden=128, num_heads=4).to(dev)
    return net, dataset.ESC_pc(x, y, np.linspace(0, 0.5, F), device=dev)


if __name__ == "__main__":
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    dist.init_process_group("gloo")
    net, ds = held_out(dev)
    ev = trainer.Evaluator(net, ds, 32, _lib.MODE_F32, topk=3, process_group=dist.group.WORLD)
    out = ev.run()
    shard = int(ev.n_local)
    sizes = [torch.zeros(1, dtype=torch.int64) for _ in range(world)]
    dist.all_gather(sizes, torch.tensor([shard]))
    if rank == 0:
        print("SHARDS", [int(s) for s in sizes], flush=True)
        torch.save({k: (v if torch.is_tensor(v) else torch.tensor(v)) for k, v in out.items()},
                   os.environ["PCA_OUT"])
    dist.barrier()
    dist.destroy_process_group()
