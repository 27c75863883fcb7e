"""Cases, runners and hashes shared by tests/test_gpu_mab1_bwd_loads.py and scripts/mab1_bwd_loads_golden.py (which
records the hashes of a given build of the library in tests/golden/mab1_bwd_loads_sha256.json).

k_mab1_bwd (csrc/mab1_bwd_bf16.hip) on the paths that tests/test_gpu_mid_prologue.py does not reach.  d = 128,
h = 4, C = 50; whole train steps of the engine on the per-block path (PCA_SET128=0), and single MAB modules for the
instances that take fp32 activations: at m = 16 no whole model reaches them (the d = 128 / m = 16 engine hands bf16
activations from block to block), at m = 32 a whole step is not reproducible from pass to pass (UNPINNED below)."""
import contextlib
import hashlib
import os

D, H, C = 128, 4, 50

# key -> (B, N, din, m, lengths, extra environment, instances of k_mab1_bwd<D, MI, WANT_DX, FUSE_KV, FUSE_WQ, ABF>
# it runs: layer 2, layer 1 - mab1_bf16_bwd_ex's dispatch)
ENGINE = {
    # a ragged last tile (rows past N inside a tile) and dZ materialised because N % 128 != 0
    "ragged-B3-N200-din2": (3, 200, 2, 16, None, {}, ("16, true, true, false, true", "16, false, true, true, true")),
    "ragged-B3-N200-din3": (3, 200, 3, 16, None, {}, ("16, true, true, false, true", "16, false, true, true, true")),
    # dZ materialised at full tiles
    "dz-B3-N256-din2": (3, 256, 2, 16, None, {"PCA_D128_DZ_MASK": "0"},
                        ("16, true, true, false, true", "16, false, true, true, true")),
    # layer 1 reads a saved Qp (mab1_saves_qp: dq = 4): neither dX nor the fc_q recomputation
    "savedqp-B2-N256-din4": (2, 256, 4, 16, None, {},
                             ("16, true, true, false, true", "16, false, true, false, true")),
    "savedqp-1wg-B1-N128-din4": (1, 128, 4, 16, None, {},
                                 ("16, true, true, false, true", "16, false, true, false, true")),
    # a set smaller than one tile: waves without a live row
    "subtile-B2-N72-din3": (2, 72, 3, 16, None, {}, ("16, true, true, false, true", "16, false, true, true, true")),
    # variable-size sets of a padded batch
    "lengths-B5-N384-din2": (5, 384, 2, 16, (384, 300, 129, 128, 1), {},
                             ("16, true, true, false, true", "16, false, true, true, true")),
    # more tiles than the 256 workgroups of the grid-stride form.  At m = 16 (the fused form) every workgroup stays
    # inside one set whatever the batch - 260 workgroups here, waves 4..7 of layer 2 without a tile; a workgroup
    # that moves on to another set, and stages the K / V images again, needs m = 32: the case after the next
    "newset-B260-N128-din2": (260, 128, 2, 16, None, {},
                              ("16, true, true, false, true", "16, false, true, true, true")),
}
# key -> (B, N, m, dq, instance): one many-queries MAB module, fp32 in and out (the exact per-block entry points)
MODULE = {
    "f32act-dx-B2-N136-dq128": (2, 136, 16, 128, "16, true, true, false, false"),
    "f32act-fcq-B2-N136-dq2": (2, 136, 16, 2, "16, false, true, true, false"),
    "f32act-qp-B2-N136-dq4": (2, 136, 16, 4, "16, false, true, false, false"),
    "f32act-qp-1wg-B1-N128-dq4": (1, 128, 16, 4, "16, false, true, false, false"),
    # m = 32: the grid-stride form without the fused K / V gradients (k_kv_grad reads dS, P, dO from memory); two
    # tiles per set, the second with 8 live rows in its first wave only.  (A whole m = 32 train step is no case:
    # outside the d = 128 / m = 16 step's slabs its weight gradients are summed by atomics, and the parent's
    # passes differ in up to 28 of the 45.)
    "m32-dx-B2-N136-dq128": (2, 136, 32, 128, "32, true, false, false, false"),
    "m32-pt-B2-N136-dq2": (2, 136, 32, 2, "32, false, false, false, false"),
    "m32-pt-1wg-B1-N128-dq2": (1, 128, 32, 2, "32, false, false, false, false"),
    # 260 one-tile sets on the 256 workgroups of that form: workgroups 0..3 go on to the tiles of sets 256..259 and
    # stage the K / V images again
    "m32-newset-B260-N128-dq128": (260, 128, 32, 128, "32, true, false, false, false"),
}


# Outputs that no build reproduces from pass to pass, so that neither the two-pass check nor a recorded hash can
# cover them; the oracle still judges them.  With dq <= 4 outside the fused layer-1 reduction the fc_q gradient of
# the block is summed over the 128-row workgroups of k_wgrad_small by fp32 atomics (csrc/terminal_bodies.hpp), in
# the order the workgroups arrive: the parent's own passes differ there once there is more than one workgroup (512
# and 272 rows here).  The -1wg cases hold the same instances of k_mab1_bwd with 128 rows, one workgroup, and pin
# every output.  With 33280 rows every weight gradient of a single block is such a sum (k_wgrad128 outside the
# step's slabs): that case pins Y, dQ - the dX that k_mab1_bwd writes itself - and dK.
_FC_Q = ("fc_q.weight", "fc_q.bias")
UNPINNED = {
    "savedqp-B2-N256-din4": ("enc.0.mab1.fc_q.weight", "enc.0.mab1.fc_q.bias"),
    "f32act-qp-B2-N136-dq4": _FC_Q,
    "m32-pt-B2-N136-dq2": _FC_Q,
    "m32-newset-B260-N128-dq128": _FC_Q + ("fc_k.weight", "fc_k.bias", "fc_v.weight", "fc_v.bias", "fc_o.weight",
                                           "fc_o.bias"),
}


def ran(names, args):
    """Whether the kernel names of a step (demangled or not) hold the instance k_mab1_bwd<D, args>."""
    vals = [a.strip() for a in args.split(",")]
    mangled = f"k_mab1_bwdILi{D}ELi{vals[0]}E" + "".join("Lb1E" if v == "true" else "Lb0E" for v in vals[1:]) + "E"
    plain = f"k_mab1_bwd<{D}, {args}>".replace(" ", "")
    return any(mangled in n or plain in n.replace(" ", "") for n in names)


@contextlib.contextmanager
def env(**kv):
    old = {k: os.environ.get(k) for k in kv}
    os.environ.update(kv)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def net_of(dev, din, m, seed):
    import models
    import torch
    torch.manual_seed(seed)
    return models.ST(dim_input=din, num_outputs=1, dim_output=C, num_inds=m, dim_hidden=D, num_heads=H).to(dev)


def engine_inputs(key):
    import inputs as gi
    B, N, din, m, lengths, _, _ = ENGINE[key]
    X = gi.pc_input(8700 + N + B, B, N, din)
    if lengths is not None:
        for b, L in enumerate(lengths):        # padding rows: zeros, as the pack kernel writes
            X[b, L:] = 0.0
    return X, gi.labels(8701 + N + B, B, C)


def engine_net(dev, key):
    B, N, din, m, _, _, _ = ENGINE[key]
    return net_of(dev, din, m, 1300 + N + din + m)


def kernel_names(fn):
    """Names of the library's device kernels that one call of fn() launches."""
    import torch
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    cuda = getattr(torch.autograd.DeviceType, "CUDA", None)
    return [e.name for e in prof.events() if e.device_type == cuda and "pca" in e.name]


def engine_run(net, key, X, y, witness=False):
    """One eager train step -> {"logits", "loss", one entry per gradient}; witness: also the kernel names of
    one more step."""
    import torch
    from pca_hip import _lib, trainer
    B, N, din, m, lengths, extra, _ = ENGINE[key]
    ld = None if lengths is None else torch.tensor(lengths, dtype=torch.int32, device=X.device)
    with env(PCA_SET128="0", **extra):
        eng = trainer.STEngine(net, B, N, _lib.MODE_BF16, training=True)
        eng.fwd_bwd(X, y, phase=-1, lengths=ld)
        torch.cuda.synchronize()
        eng.check_handoffs()
        out = {"logits": eng.logits.clone(), "loss": eng.loss.clone()}
        g = eng.grads.clone()
        off = 0
        for k, prm in net.named_parameters():
            out[k] = g[off:off + prm.numel()].view_as(prm)
            off += prm.numel()
        assert off == g.numel() and len(out) == 47, (off, g.numel(), len(out))
        names = kernel_names(lambda: eng.fwd_bwd(X, y, phase=-1, lengths=ld)) if witness else None
    return out, names


def engine_oracle(net, key, Xn, yn):
    """loss, logits [B, C] and gradients of the CPU oracle (on X[b, :lengths[b]] where there are lengths)."""
    import torch
    from oracle import st_oracle as orc
    B, N, din, m, lengths, _, _ = ENGINE[key]
    p = {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}
    if lengths is None:
        loss, lg, g = orc.st_grads(torch.from_numpy(Xn), torch.from_numpy(yn), p, H)
        return loss, lg.reshape(B, C), g
    params = {k: v.requires_grad_(True) for k, v in p.items()}
    lg = torch.cat([orc.st_forward(torch.from_numpy(Xn[b:b + 1, :lengths[b]]), params, H).reshape(1, -1)
                    for b in range(B)], 0)
    loss = orc.cross_entropy(lg, torch.from_numpy(yn))
    loss.backward()
    return float(loss.detach()), lg.detach(), {k: v.grad for k, v in params.items()}


def module_inputs(key):
    """Points or activations X [B, N, dq], the block's keys K [B, m, d], the upstream gradient G [B, N, d] and
    the block's parameters, host tensors."""
    import numpy as np
    import torch
    B, N, m, dq, _ = MODULE[key]
    g = torch.Generator().manual_seed(1700 + N + dq)
    X = torch.randn(B, N, dq, generator=g)
    if dq <= 4:
        X[..., -1] = X[..., -1] * 3 - 9                      # log-magnitude-like column
    K = torch.randn(B, m, D, generator=g)
    G = torch.randn(B, N, D, generator=g)
    p = {}
    for nm, din in (("fc_q", dq), ("fc_k", D), ("fc_v", D), ("fc_o", D)):
        bound = 1.0 / np.sqrt(din)
        p[nm + ".weight"] = (torch.rand(D, din, generator=g) * 2 - 1) * bound
        p[nm + ".bias"] = (torch.rand(D, generator=g) * 2 - 1) * bound
    return X, K, G, p


def module_run(dev, key, witness=False):
    """Forward and backward of the module in bf16 mode -> {"Y", "dQ" (dq > 4), "dK", one entry per parameter}."""
    import modules
    import pca_hip
    import torch
    B, N, m, dq, _ = MODULE[key]
    X, K, G, p = module_inputs(key)
    mab = modules.MAB(dq, D, D, H)
    mab.load_state_dict(p)
    mab = mab.to(dev)
    Qd = X.to(dev).requires_grad_(dq > 4)
    Kd = K.to(dev).requires_grad_(True)
    Gd = G.to(dev)

    def step():
        Y = mab(Qd, Kd, q_shared=False)
        (Y * Gd).sum().backward()
        return Y

    pca_hip.set_mode("bf16")
    try:
        Y = step()
        torch.cuda.synchronize()
        out = {"Y": Y.detach().clone(), "dK": Kd.grad.clone()}
        if dq > 4:
            out["dQ"] = Qd.grad.clone()
        for k, prm in mab.named_parameters():
            out[k] = prm.grad.clone()
        names = kernel_names(step) if witness else None
    finally:
        pca_hip.set_mode("f32")
    return out, names


def module_oracle(key):
    from oracle import st_oracle as orc
    X, K, G, p = module_inputs(key)
    ref = orc.mab_backward(G, X, K, p, H)
    ref["Y"] = orc.mab_forward(X, K, p, H)
    return ref


def module_emulation(key):
    """Gradients by autograd through the bf16 operand emulation of the block (oracle/st_oracle.py): the same ReLU
    masks as the kernels', so a wrong tile cannot hide behind a flipped derivative."""
    from oracle import st_oracle as orc
    B, N, m, dq, _ = MODULE[key]
    X, K, G, p = module_inputs(key)
    leaves = {k: v.clone().requires_grad_(True) for k, v in p.items()}
    Xe, Ke = X.clone().requires_grad_(True), K.clone().requires_grad_(True)
    (orc.mab1_forward_bf16emu(Xe, Ke, leaves, H) * G).sum().backward()
    emu = {k: v.grad for k, v in leaves.items()}
    emu["dQ"], emu["dK"] = Xe.grad, Ke.grad
    return emu


def _sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def hashes(out):
    """SHA-256 of the bytes of every output."""
    return {k: _sha(v) for k, v in out.items()}
