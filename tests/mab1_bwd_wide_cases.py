"""Cases and runners shared by tests/test_gpu_mab1_bwd_wide.py and scripts/mab1_bwd_wide_golden.py (which records
the hashes of a given build of the library in tests/golden/mab1_bwd_wide_sha256.json).

k_mab1_bwd (csrc/mab1_bwd_bf16.hip) where a tile operand that moves as 16-byte pieces, or a wave's points that
move as one contiguous block, could touch a byte outside its tile: whole eager train steps, d = 128, h = 4, m = 16,
C = 50, bf16 mode.  engine_run / hashes / ran / env / kernel_names come from mab1_bwd_loads_cases."""
import contextlib

import mab1_bwd_loads_cases as lc

D, H, M, C = lc.D, lc.H, 16, lc.C
_L2, _L1 = "16, true, true, false, true", "16, false, true, true, true"

# key -> (B, N, din, set-resident forward, instances of k_mab1_bwd<D, MI, WANT_DX, FUSE_KV, FUSE_WQ, ABF>: layer 2,
# layer 1)
CASES = {
    # the last tile has one live row; N % 128 != 0, so dZ is materialised and its store runs
    "last-row-B2-N129-din2": (2, 129, 2, False, (_L2, _L1)),
    # one full 16-row group plus one row; the points block of a wave is 96 floats, 3 of them valid in wave 1
    "group-plus-one-B2-N33-din3": (2, 33, 3, False, (_L2, _L1)),
    # a set of half a wave's 32 points: one 16-row group, the second group and waves 1..3 without a live row
    "one-group-B3-N16-din2": (3, 16, 2, False, (_L2, _L1)),
    # a single component per point
    "one-component-B1-N40-din1": (1, 40, 1, False, (_L2, _L1)),
    # the set-resident forward hands bf16 tensors to both launches
    "set128-B5-N256-din2": (5, 256, 2, True, (_L2, _L1)),
}
# the cases that run again with X inside a larger NaN tensor and with the workspace filled with 0xFF bytes
SURROUNDED = ("last-row-B2-N129-din2", "group-plus-one-B2-N33-din3")
PAD = 64          # floats of NaN directly before and after X (256 bytes: X keeps the alignment of an allocation)

# Words of the engine's workspace that the host initialises by contract, so that the 0xFF fill leaves them alone:
# the hand-off counter of the set-resident forward (trainer.STEngine._handoff_word; only the caller clears it).
# There is no other: everything else in the workspace is written by the step before it is read.


def engine_net(dev, key):
    B, N, din = CASES[key][:3]
    return lc.net_of(dev, din, M, 2100 + N + din)


def engine_inputs(key):
    import inputs as gi
    B, N, din = CASES[key][:3]
    return gi.pc_input(9300 + N + B, B, N, din), gi.labels(9301 + N + B, B, C)


def surrounded(Xn, dev):
    """X as a slice in the middle of a larger tensor that is NaN directly before and after it."""
    import torch
    buf = torch.full((PAD + Xn.size + PAD,), float("nan"), dtype=torch.float32, device=dev)
    X = buf[PAD:PAD + Xn.size].view(*Xn.shape)
    X.copy_(torch.from_numpy(Xn))
    assert X.is_contiguous() and X.data_ptr() == buf.data_ptr() + 4 * PAD
    assert bool(torch.isnan(buf[:PAD]).all()) and bool(torch.isnan(buf[PAD + Xn.size:]).all())
    return X, buf


@contextlib.contextmanager
def _registered(key):
    """engine_run looks its case up in lc.ENGINE: the case is entered for the call alone (the parametrisation of
    tests/test_gpu_mab1_bwd_loads.py, made at collection, never sees it)."""
    B, N, din, set128, inst = CASES[key]
    assert not set128 and key not in lc.ENGINE
    lc.ENGINE[key] = (B, N, din, M, None, {}, inst)
    try:
        yield
    finally:
        del lc.ENGINE[key]


def run(net, key, X, y, witness=False, fill_ws=False):
    """One eager train step -> ({"logits", "loss", one entry per gradient}, kernel names of one more step or None).
    fill_ws: the engine's workspace is filled with 0xFF bytes before the step, the hand-off counter word apart."""
    import torch
    from pca_hip import _lib, trainer
    B, N, din, set128, _ = CASES[key]
    if not set128 and not fill_ws:
        with _registered(key):
            return lc.engine_run(net, key, X, y, witness=witness)
    with lc.env(PCA_SET128="1" if set128 else "0"):
        eng = trainer.STEngine(net, B, N, _lib.MODE_BF16, training=True)
        if fill_ws:
            eng.ws.fill_(0xFF)
            if eng._handoff_word is not None:
                eng._handoff_word.zero_()
        eng.fwd_bwd(X, y, phase=-1)
        torch.cuda.synchronize()
        eng.check_handoffs()
        out = {"logits": eng.logits.clone(), "loss": eng.loss.clone()}
        g = eng.grads.clone()
        off = 0
        for k, prm in net.named_parameters():
            out[k] = g[off:off + prm.numel()].view_as(prm)
            off += prm.numel()
        assert off == g.numel() and len(out) == 47, (off, g.numel(), len(out))
        names = lc.kernel_names(lambda: eng.fwd_bwd(X, y, phase=-1)) if witness else None
    return out, names


def oracle(net, key, Xn, yn):
    """loss, logits [B, C] and gradients of the CPU oracle."""
    import torch
    from oracle import st_oracle as orc
    B = CASES[key][0]
    p = {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}
    loss, lg, g = orc.st_grads(torch.from_numpy(Xn), torch.from_numpy(yn), p, H)
    return loss, lg.reshape(B, C), g
