"""Cases and the runner shared by tests/test_gpu_set128_addr.py and scripts/set128_addr_golden.py (which records
the hashes of a given build of the library in tests/golden/set128_addr_sha256.json).

k_set128_fwd (csrc/set128_fwd.hip) where an address can go wrong once every global access is a scalar base plus
a 32-bit lane offset, the saved Qp leaves in 16-byte chunks and the ReLU mask as whole words: whole eager train
steps, d = 128, h = 4, m = 16, C = 50, bf16 mode, on the set-resident path.  B below, at and across the 8-wide
grouping of the workgroup pairs, both N (one and two units per quad), every layer-1 width (din = 4: layer 1 saves
its Qp too), each dense and with ``lengths`` that hold 1, N / 2 and N."""
import ctypes as C

import mab1_bwd_loads_cases as lc

D, H, M, NC = lc.D, lc.H, 16, lc.C

# key -> (B, N, din, lengths or None).  The B = 1 case comes first.
_SHAPES = [(1, 256, 1), (2, 256, 2), (9, 256, 3), (3, 512, 4), (5, 512, 2)]
_LENGTHS = {
    (1, 256, 1): [128],
    (2, 256, 2): [1, 256],
    (9, 256, 3): [256, 1, 128, 129, 127, 33, 31, 2, 256],
    (3, 512, 4): [1, 256, 512],
    (5, 512, 2): [512, 1, 256, 257, 97],
}
CASES = {}
for _s in _SHAPES:
    CASES["dense-B%d-N%d-din%d" % _s] = (*_s, None)
for _s in _SHAPES:
    CASES["lengths-B%d-N%d-din%d" % _s] = (*_s, _LENGTHS[_s])
# the cases that run again with X inside a larger NaN tensor and with the workspace filled with 0xFF bytes
SURROUNDED = ("dense-B2-N256-din2", "dense-B5-N512-din2")
PAD = 64          # floats of NaN directly before and after X (256 bytes: X keeps the alignment of an allocation)
N_OUT = 47        # logits, loss, 45 gradients
# Outputs that are not pinned, and not compared between passes: at din = 4 layer 1's backward reads the saved Qp
# and its fc_q weight and bias gradients are summed by atomics - three passes of the parent's library differ in
# exactly these two (scripts/set128_addr_golden.py refuses any other), as tests/mab1_bwd_loads_cases.py has it
# for its din = 4 case.  The saved Qp of layer 1 itself is pinned.
_FC_Q1 = ("enc.0.mab1.fc_q.weight", "enc.0.mab1.fc_q.bias")
UNPINNED = {k: _FC_Q1 for k, v in CASES.items() if v[2] == 4}


def engine_net(dev, key):
    B, N, din, _ = CASES[key]
    return lc.net_of(dev, din, M, 5200 + N + din)


def engine_inputs(key):
    import inputs as gi
    B, N, din, lengths = CASES[key]
    X = gi.pc_input(9500 + N + B, B, N, din)
    if lengths is not None:
        for b, L in enumerate(lengths):        # padding rows: zeros, as the pack kernel writes
            X[b, L:] = 0.0
    return X, gi.labels(9501 + N + B, B, NC)


def surrounded(Xn, dev):
    """X as a slice in the middle of a larger tensor that is NaN directly before and after it."""
    import torch
    buf = torch.full((PAD + Xn.size + PAD,), float("nan"), dtype=torch.float32, device=dev)
    X = buf[PAD:PAD + Xn.size].view(*Xn.shape)
    X.copy_(torch.from_numpy(Xn))
    assert X.is_contiguous() and X.data_ptr() == buf.data_ptr() + 4 * PAD
    return X, buf


def _a256(n):
    return (n + 255) & ~255


def saved_tensors(eng, B, N, din):
    """Byte views of what the set-resident forward saved for the backward: the many-queries blocks' Qp (layer 2;
    layer 1 where din = 4), O and ReLU mask words, and the output of layer 1.  Offsets: pca_st_ws_layout and the
    carve order of mab1_carve_saved (KpP, VpP, Kt, Vt, QpS, OS, mask, each 256-aligned)."""
    from pca_hip import _lib
    lay = (C.c_int64 * 11)()
    _lib.check(_lib.lib().pca_st_ws_layout(C.byref(eng.cfg), C.cast(lay, C.c_void_p)), "pca_st_ws_layout")
    lay = list(lay)
    kv, act, msk = _a256(B * M * D * 2), B * N * D * 2, B * N * 16
    out = {}
    for li, base, end in ((1, lay[1], lay[2]), (2, lay[3], lay[4])):
        qps = base + 4 * kv
        os_ = qps + _a256(act)
        mk = os_ + _a256(act)
        assert mk + msk <= end, (li, base, end, mk + msk)
        if li == 2 or din == 4:
            out["saved.QpS%d" % li] = eng.ws[qps:qps + act]
        out["saved.OS%d" % li] = eng.ws[os_:os_ + act]
        out["saved.mask%d" % li] = eng.ws[mk:mk + msk]
    out["saved.Y1"] = eng.ws[lay[7]:lay[7] + act]
    return {k: v.clone() for k, v in out.items()}


def run(net, key, X, y, witness=False, fill_ws=False):
    """One eager train step -> ({"logits", "loss", one entry per gradient, the saved tensors}, kernel names of one
    more step or None).  fill_ws: the engine's workspace is filled with 0xFF bytes before the step, the hand-off
    counter word apart."""
    import torch
    from pca_hip import _lib, trainer
    B, N, din, lengths = CASES[key]
    ld = None if lengths is None else torch.tensor(lengths, dtype=torch.int32, device=X.device)
    with lc.env(PCA_SET128="1"):
        eng = trainer.STEngine(net, B, N, _lib.MODE_BF16, training=True)
        if fill_ws:
            eng.ws.fill_(0xFF)
            if eng._handoff_word is not None:
                eng._handoff_word.zero_()
        eng.fwd_bwd(X, y, phase=-1, lengths=ld)
        torch.cuda.synchronize()
        eng.check_handoffs()
        assert eng._handoff_word is not None and int(eng._handoff_word.item()) == 0
        out = {"logits": eng.logits.clone(), "loss": eng.loss.clone()}
        g = eng.grads.clone()
        off = 0
        for k, prm in net.named_parameters():
            out[k] = g[off:off + prm.numel()].view_as(prm)
            off += prm.numel()
        assert off == g.numel() and len(out) == N_OUT, (off, g.numel(), len(out))
        out.update(saved_tensors(eng, B, N, din))
        names = lc.kernel_names(lambda: eng.fwd_bwd(X, y, phase=-1, lengths=ld)) if witness else None
        if witness:
            eng.check_handoffs()
    return out, names
