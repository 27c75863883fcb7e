"""The d = 64 training step (the reference's shipped shape: ST(dim_hidden=64, num_heads=8, num_inds=64)) in the
bf16 mode is bit-reproducible: csrc/wgrad64.hip writes per-workgroup slabs, k_slab_sum_jobs adds them in a
fixed order, one launch per block, and nothing else in the step adds in fp32 with atomics.

1. The weight-gradient calls of the four block shapes of the step - many queries (nq = N, nk = 64) with
   dq = 2 / 3 and dq = 64, shared few queries (nq = 64, nk = N) with dk = 2 / 3 and dk = 64, and the PMA - at
   M = 3075 rows (193 row groups, the last with 3 live rows, 13 workgroups) and M = 32 800 (2050 groups: the
   128-workgroup cap and a second trip for two waves): two calls from identically prefilled gradient buffers
   are bitwise equal, and result - prefill equals the zero-prefilled result within one fp32 addition.
   These shapes run through STEngine.fwd_bwd: pca_mab_bwd refuses a d = 64 block that is not
   self-attention-shaped in PCA_MODE_BF16 (tests/test_sab_host.py pins its size queries at 0), so the
   engine call is the entry that reaches mab_f32_bwd with them.
2. The FST, 3ST and padded steps: three calls on fresh engines agree bitwise in logits, loss, statistics
   and gradients; the first also meets the bars of test_shipped_shape_train_step_fused_core.
3. Trainer at the FST shape: hipGraph replay = eager launches over 4 steps, and 6 steps straight = 3 steps,
   a checkpoint through runfiles, a new Trainer, 3 steps - parameters, Adam moments, statistics.
4. STEngine.bit_reproducible / Trainer.bit_reproducible (pca_st_step_reproducible) say so, and every engine
   that says True repeats itself bit for bit."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

# din, d, h, m, C, B, N, lengths
FST = (2, 64, 8, 64, 10, 6, 1025, None)
ST3 = (3, 64, 8, 64, 10, 3, 5120, None)
PADDED = (2, 64, 8, 64, 10, 4, 300, [300, 129, 17, 1])
STEP_CASES = [FST, ST3, PADDED]


@pytest.fixture(scope="module")
def dev():
    import pca_hip
    pca_hip.lib()
    yield torch.device("cuda", 0)
    pca_hip.set_mode("f32")


def _bits(t):
    t = t.detach()
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _net(dev, din, d, h, m, C, seed):
    import models
    torch.manual_seed(seed)
    return models.ST(dim_input=din, num_outputs=1, dim_output=C, num_inds=m, dim_hidden=d, num_heads=h).to(dev)


def _inputs(case, dev):
    """Net, X, labels and lengths of a case: the seeds and generators of tests/test_gpu_sd64.py."""
    import inputs as gi
    from util import T
    din, d, h, m, C, B, N, lengths = case
    net = _net(dev, din, d, h, m, C, 77 + N)
    X = gi.pc_input(880 + N, B, N, din)
    y = gi.labels(881 + N, B, C)
    ld = None
    if lengths is not None:
        for b, L in enumerate(lengths):
            X[b, L:] = 0.0
        ld = torch.tensor(lengths, dtype=torch.int32, device=dev)
    return net, X, y, T(X, dev), T(y, dev), ld


def _call(net, case, Xd, yd, ld, mode, prefill=None):
    """One fwd_bwd on a FRESH engine (its gradient vector zero, or ``prefill``); clones of the results."""
    from pca_hip import trainer
    B, N = case[5], case[6]
    eng = trainer.STEngine(net, B, N, mode, training=True)
    if prefill is not None:
        eng.grads.copy_(prefill)
    eng.fwd_bwd(Xd, yd, lengths=ld)
    torch.cuda.synchronize()
    return dict(logits=eng.logits.clone(), loss=eng.loss.clone(), stats=eng.stats.clone(),
                grads=eng.grads.clone()), eng


def _assert_same(a, b, what):
    for k in ("logits", "loss", "stats", "grads"):
        x, y = _bits(a[k]), _bits(b[k])
        assert torch.equal(x, y), f"{what}: {k} differs in {int((x != y).sum())} of {x.numel()} elements"


# ---- 1. the weight-gradient calls of every block shape, accumulate contract ------------------------------------
# din, B: N = 1025, so M = B N = 3075 (13 workgroups, ragged last group) and 32 800 (the 128-workgroup cap)
WGRAD_CASES = [(2, 3), (3, 3), (2, 32), (3, 32)]


@pytest.mark.parametrize("din,B", WGRAD_CASES, ids=[f"din{a}_B{b}" for a, b in WGRAD_CASES])
def test_weight_gradients_accumulate_in_a_fixed_order(dev, din, B):
    import inputs as gi
    from pca_hip import _lib
    from util import T
    case = (din, 64, 8, 64, 10, B, 1025, None)
    net, _, _, Xd, yd, _ = _inputs(case, dev)
    n = sum(p.numel() for p in net.parameters())
    P = T(gi.randn(4100 + 10 * din + B, n).astype(np.float32) * 0.05, dev)      # non-zero everywhere
    assert float(P.abs().min()) > 0
    a, _ = _call(net, case, Xd, yd, None, _lib.MODE_BF16, prefill=P)
    b, _ = _call(net, case, Xd, yd, None, _lib.MODE_BF16, prefill=P)
    z, _ = _call(net, case, Xd, yd, None, _lib.MODE_BF16)
    _assert_same(a, b, f"din {din} B {B}, two calls onto the same prefill")
    acc, fresh, p64 = a["grads"].double().cpu(), z["grads"].double().cpu(), P.double().cpu()
    assert torch.isfinite(acc).all() and float(fresh.abs().max()) > 0
    off, checked = 0, 0
    for name, prm in net.named_parameters():
        sl = slice(off, off + prm.numel())
        off += prm.numel()
        if ".fc_" not in name:          # I, S, dec.1: not weight-gradient calls of a block
            continue
        delta = ((acc[sl] - p64[sl]) - fresh[sl]).abs()
        lim = 2.0 ** -23 * (p64[sl].abs() + fresh[sl].abs())
        worst = float((delta / lim).max())
        print(f"din {din} B {B} {name}: worst |acc - P - fresh| = {worst:.3f} x 2^-23 (|P| + |fresh|)")
        assert bool((delta <= lim).all()), (name, worst)
        checked += 1
    assert checked == 40                # 5 blocks x (4 weights + 4 biases)


# ---- 2. the whole step -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", STEP_CASES, ids=["fst", "3st", "padded"])
def test_step_repeats_bitwise_and_meets_the_oracle(dev, case):
    import grad_bars as gb
    from oracle import st_oracle as orc
    from pca_hip import _lib
    from util import close
    din, d, h, m, C, B, N, lengths = case
    net, X, y, Xd, yd, ld = _inputs(case, dev)
    runs = [_call(net, case, Xd, yd, ld, _lib.MODE_BF16)[0] for _ in range(3)]
    for i in (1, 2):
        _assert_same(runs[0], runs[i], f"{case[:7]} call 0 vs call {i}")
    p = {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}
    if lengths is None:
        ref_loss, ref_lg, ref_g = orc.st_grads(torch.from_numpy(X), torch.from_numpy(y), p, h)
    else:
        params = {k: v.clone().requires_grad_(True) for k, v in p.items()}
        lg = torch.cat([orc.st_forward(torch.from_numpy(X[b:b + 1, :lengths[b]]), params, h).reshape(1, -1)
                        for b in range(B)], 0)
        loss = orc.cross_entropy(lg, torch.from_numpy(y))
        loss.backward()
        ref_loss, ref_lg, ref_g = float(loss), lg.detach(), {k: v.grad for k, v in params.items()}
    first = runs[0]
    close(first["logits"], ref_lg.reshape(B, C), 3e-2, "logits")
    assert abs(float(first["loss"]) - ref_loss) < 3e-2 * max(1.0, abs(ref_loss))
    gb.judge(first["grads"], ref_g, gb.BF16_VS_ORACLE, gb.shapes_of(net), f"d={d} N={N} vs oracle")


# ---- 3. Trainer: graph = eager, exact resume ---------------------------------------------------------------------
def _fst_dataset(dev, T=25, F=1025, C=10, seed=41):
    """25 sets of 1025 points (f, logmag): 4 steps of 6 sets per epoch."""
    import dataset
    rng = np.random.Generator(np.random.PCG64(seed))
    x = rng.normal(-9, 3, size=(F, T)).astype(np.float32)
    y = rng.integers(0, C, size=(T,))
    return dataset.ESC_pc(x, y, np.linspace(0, 0.5, F), device=dev)


def _fst_trainer(dev, ds, graph):
    from pca_hip import _lib, trainer
    net = _net(dev, 2, 64, 8, 64, 10, seed=3)
    return trainer.Trainer(net, ds, 6, mode=_lib.MODE_BF16, use_graph=graph, seed=1, keep_grads=True)


def _state(tr):
    torch.cuda.synchronize()
    return (tr.eng.flat.clone(), tr.m.clone(), tr.v.clone(), tr.step_count.clone(), tr.eng.stats.clone())


def _same_bits(a, b, what):
    for x, y, name in zip(a, b, ("parameters", "m", "v", "step_count", "statistics")):
        xi, yi = _bits(x), _bits(y)
        assert torch.equal(xi, yi), f"{what}: {name} not bitwise equal ({int((xi != yi).sum())} elements differ)"


def test_trainer_graph_equals_eager_bitwise(dev):
    ds = _fst_dataset(dev)
    assert ds.num_points == 1025

    def run(graph):
        tr = _fst_trainer(dev, ds, graph)
        assert tr.bit_reproducible
        for _ in range(4):
            tr.step()
        return _state(tr) + (tr.eng.grads.clone(),)

    g, e = run(True), run(False)
    assert torch.isfinite(g[0]).all() and int(g[3][0]) == 4 and float(g[5].abs().max()) > 0
    _same_bits(g[:5], e[:5], "hipGraph replay vs eager launches")
    assert torch.equal(_bits(g[5]), _bits(e[5])), "gradients of the last step"


def test_trainer_resumes_bitwise(dev, tmp_path):
    import runfiles
    ds = _fst_dataset(dev)
    K = 3
    straight = _fst_trainer(dev, ds, True)
    for _ in range(2 * K):
        straight.step()
    want = _state(straight)
    assert torch.isfinite(want[0]).all() and int(want[3][0]) == 2 * K
    first = _fst_trainer(dev, ds, True)
    for _ in range(K):
        first.step()
    spe = first.indices.steps_per_epoch()
    assert K % spe and (2 * K) // spe > K // spe              # mid-epoch, and an epoch boundary follows
    path = str(tmp_path / "fst.ckpt")
    runfiles.save_checkpoint(path, first, config=dict(note="d = 64 resume"))
    half = _state(first)
    del first
    second = _fst_trainer(dev, ds, True)
    with torch.no_grad():
        second.eng.flat.add_(1.0)                             # not the saved weights
    assert runfiles.load_checkpoint(path, second)["note"] == "d = 64 resume"
    _same_bits(_state(second), half, "after load_checkpoint")
    for _ in range(K):
        second.step()
    _same_bits(_state(second), want, "3 steps + checkpoint + 3 steps vs 6 steps")


# ---- 4. the interface ---------------------------------------------------------------------------------------------
TINY_128 = (2, 128, 4, 16, 10, 4, 128, None)                  # cfg2's architecture
TINY_256 = (2, 256, 8, 32, 10, 2, 128, None)


@pytest.mark.parametrize("case", STEP_CASES + [TINY_128, TINY_256], ids=["fst", "3st", "padded", "d128", "d256"])
def test_bit_reproducible_is_true_and_holds(dev, case):
    from pca_hip import _lib
    net, _, _, Xd, yd, ld = _inputs(case, dev)
    a, eng = _call(net, case, Xd, yd, ld, _lib.MODE_BF16)
    assert eng.reproducible(ld is not None) is True
    if ld is None:
        assert eng.bit_reproducible is True
    assert _lib.lib().pca_st_step_reproducible(C.byref(eng.cfg), int(ld is not None)) == 1
    b, _ = _call(net, case, Xd, yd, ld, _lib.MODE_BF16)
    _assert_same(a, b, f"{case[:7]}: bit_reproducible says True")
    assert torch.isfinite(a["grads"]).all() and float(a["grads"].abs().max()) > 0


def test_bit_reproducible_is_false_where_nothing_is_promised(dev):
    from pca_hip import _lib, trainer
    L = _lib.lib()
    for case in STEP_CASES + [TINY_128, TINY_256]:
        din, d, h, m, Cc, B, N, lengths = case
        net = _net(dev, din, d, h, m, Cc, 1)
        assert trainer.STEngine(net, B, N, _lib.MODE_F32, training=True).bit_reproducible is False
    # the sum over sets of the shared queries' gradient is atomic-free up to 256 sets only
    assert L.pca_st_step_reproducible(C.byref(_lib.StConfig(256, 1025, 2, 64, 8, 64, 1, 10, _lib.MODE_BF16)), 0) == 1
    assert L.pca_st_step_reproducible(C.byref(_lib.StConfig(257, 1025, 2, 64, 8, 64, 1, 10, _lib.MODE_BF16)), 0) == 0
    # another chain width, a head dim the fused core does not take
    assert L.pca_st_step_reproducible(C.byref(_lib.StConfig(4, 77, 3, 32, 8, 24, 1, 10, _lib.MODE_BF16)), 0) == 0
    assert L.pca_st_step_reproducible(C.byref(_lib.StConfig(4, 300, 2, 64, 2, 64, 1, 10, _lib.MODE_BF16)), 0) == 0
