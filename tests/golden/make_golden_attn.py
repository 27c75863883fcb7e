#!/usr/bin/env python3
"""golden_attn.npz, golden_attn_fst.npz, golden_attn_tst.npz: the pooling attention `A` of the REAL
reference on CPU (three files: none may pass 1 MiB).

Run in the build container only: ``python tests/golden/make_golden_attn.py``.
`A` is what set_transformer-master/modules.py:21-28 builds inside MAB.forward and drops; here the
reference's own ``PMA.forward`` runs unchanged - its ``fc_q``, ``fc_k``, head split, ``bmm`` and ``softmax`` -
and the softmax result is recorded, in float32 (``A``) and on a ``.double()`` copy (``A64``), and stored in the
library's layout [B, k, h, N] (the reference's [h B, k, N] row (j B + b, s) is A[b, s, j, :]).
``err_ref`` = max over rows of max_n |A - A64| / max_n A64: the reference's own float32 error, the unit of
the tests' bars.  Inputs are regenerated from seeds by the tests (inputs_attn.py).

Cases
  block/<name>   one PMA with seeded weights, S and fc_k.weight scaled by ``gain`` (a power of two) until the
                 map is peaked; dense batch of 2 sets + the lengths variant (B = 3: full, one point, cut)
  fst, tst       the shipped checkpoints (golden_ckpt.npz).  The block input is float32(enc64(X)): the
                 reference's encoder on a .double() copy, rounded once - the tests rebuild it with
                 tests/attn_ref.py instead of storing 3.7 MB.  ``err_enc``: the map's error when the encoder
                 itself runs in float32 (the reference's own float32 forward against A64); ``logits``: the
                 reference's float32 logits.
The peakedness the tests rely on is asserted here: with N >= 65 at least half of the (set, seed, head) rows
have max A N >= 8."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("PCA_REFERENCE", "/root/reference")
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(REF, "set_transformer-master"))
sys.path.insert(0, os.path.join(REF, "Code"))
os.chdir(os.path.join(REF, "Code"))

import inputs_attn as ga  # noqa: E402
import attn_ref  # noqa: E402
import modules as ref_modules  # noqa: E402  (reference)
import models as ref_models  # noqa: E402    (reference)

torch.set_num_threads(8)


def ref_A(pma, X):
    """The `A` of the reference's own MAB.forward (modules.py:28) -> [B, k, h, N] numpy: the reference's PMA
    runs unchanged and the result of its one torch.softmax call is recorded on the way."""
    grabbed = []
    real = torch.softmax

    def spy(*args, **kwargs):
        r = real(*args, **kwargs)
        grabbed.append(r)
        return r

    torch.softmax = spy
    try:
        with torch.no_grad():
            pma(X)
    finally:
        torch.softmax = real
    (A,) = grabbed
    return attn_ref.from_reference_layout(A.numpy(), X.size(0), pma.mab.num_heads)


def peaked_rows(A64):
    N = A64.shape[-1]
    return float(((A64.max(axis=-1) * N) >= 8).mean())


def both(pma, pma64, X):
    """(A, A64, err_ref) of one dense batch X (float32 tensor)."""
    A, A64 = ref_A(pma, X), ref_A(pma64, X.double())
    return A, A64, attn_ref.row_err(A, A64)


def lengths_part(out, pre, pma, pma64, Xd, mid=None):
    """The lengths variant of a dense batch Xd [>= 2, N, d]: the reference on each truncated set."""
    N = Xd.shape[1]
    src, lens = ga.lengths_variant(N, mid)
    out[pre + "len/lengths"] = lens
    errs = []
    for b, (s, n) in enumerate(zip(src, lens)):
        A, A64, e = both(pma, pma64, Xd[s:s + 1, :n])
        errs.append(e)
        if n == N:
            # the dense set again (alone in its batch: the float64 sums may differ in the last bit)
            assert np.allclose(A64[0], out[pre + "A64"][s], rtol=1e-12, atol=0)
        elif n == 1:
            assert np.all(A == 1.0) and np.all(A64 == 1.0)             # one key: exactly 1
        else:
            out[pre + f"len/A{b}"], out[pre + f"len/A64_{b}"] = A[0], A64[0]
    out[pre + "len/err_ref"] = np.array(errs, dtype=np.float64)


def gen_block():
    out = {}
    for name, d, h, N, k in ga.BLOCK_CASES:
        gain = 1.0
        while True:
            c = ga.block_case(name, gain)
            pma = ref_modules.PMA(d, h, k)
            with torch.no_grad():
                pma.S.copy_(torch.from_numpy(c["S"])[None])
                pma.mab.fc_q.weight.copy_(torch.from_numpy(c["wq"]))
                pma.mab.fc_q.bias.copy_(torch.from_numpy(c["bq"]))
                pma.mab.fc_k.weight.copy_(torch.from_numpy(c["wk"]))
                pma.mab.fc_k.bias.copy_(torch.from_numpy(c["bk"]))
            pma64 = ref_modules.PMA(d, h, k).double()
            pma64.load_state_dict({n: v.double() for n, v in pma.state_dict().items()})
            X = torch.from_numpy(c["X"])
            A, A64, err = both(pma, pma64, X)
            if N >= 65:
                done = peaked_rows(A64) >= 0.5
            elif N > 1:
                done = float((A64.max(axis=-1) >= 0.5).mean()) >= 0.5
            else:
                done = True
            if done:
                break
            gain *= 2.0
            assert gain <= 1024.0, name
        if N >= 65:
            assert peaked_rows(A64) >= 0.5, name
        pre = f"block/{name}/"
        out[pre + "gain"] = np.float64(gain)
        out[pre + "A"], out[pre + "A64"], out[pre + "err_ref"] = A, A64, np.float64(err)
        lengths_part(out, pre, pma, pma64, X)
        print(f"{name}: gain {gain:g} peaked rows {peaked_rows(A64):.2f} max A N {A64.max() * N:.1f} "
              f"err_ref {err:.3g}")
    np.savez_compressed(os.path.join(HERE, "golden_attn.npz"), **out)
    print("golden_attn.npz", len(out), "arrays")


def gen_shipped():
    ck = np.load(os.path.join(HERE, "golden_ckpt.npz"))
    a = ga.SHIPPED_ARCH
    for tag, (prefix, din, B, N, seed, mid) in ga.SHIPPED.items():
        sd = {k[len(prefix):]: torch.from_numpy(ck[k]) for k in ck.files if k.startswith(prefix)}
        net = ref_models.ST(dim_input=din, dim_hidden=a["d"], num_heads=a["h"], num_inds=a["m"])
        net.load_state_dict(sd)
        net64 = ref_models.ST(dim_input=din, dim_hidden=a["d"], num_heads=a["h"],
                              num_inds=a["m"]).double()
        net64.load_state_dict({k: v.double() for k, v in sd.items()})
        X = torch.from_numpy(ga.shipped_input(tag))
        out = {}
        with torch.no_grad():
            Y64 = net64.enc(X.double())
            Xb = Y64.float()                                   # the block input: rounded once
            Y32 = net.enc(X)                                   # the reference's own float32 encoder
            out["logits"] = net(X).numpy()
            out["logits64"] = net64(X.double()).numpy()
        # the tests rebuild Xb with the numpy encoder: same values up to a rare last-bit rounding
        Xb_np = attn_ref.shipped_block_input(X.numpy(), {k: v.numpy() for k, v in sd.items()}, a["h"])
        flips = int((Xb_np != Xb.numpy()).sum())
        assert flips <= 8, flips                               # (measured: 0 of 262 400 and 2 of 655 360)
        A, A64, err = both(net.dec[0], net64.dec[0], Xb)
        A_full = ref_A(net.dec[0], Y32)
        out["A"], out["A64"], out["err_ref"] = A, A64, np.float64(err)
        out["err_enc"] = np.float64(attn_ref.row_err(A_full, A64))
        assert peaked_rows(A64) >= 0.5, tag
        heads = (A64.max(axis=-1) * N >= 16).any(axis=(0, 1)).sum()
        lengths_part(out, "", net.dec[0], net64.dec[0], Xb, mid)
        np.savez_compressed(os.path.join(HERE, f"golden_attn_{tag}.npz"), **out)
        print(f"golden_attn_{tag}.npz: heads with max A N >= 16: {heads} of {a['h']}, peak A N "
              f"{A64.max() * N:.0f}, err_ref {err:.3g}, err_enc {out['err_enc']:.3g}, input flips {flips}")


if __name__ == "__main__":
    gen_block()
    gen_shipped()
