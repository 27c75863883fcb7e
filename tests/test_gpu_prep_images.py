"""The image and clear items of the preparation plan on the device (csrc/prep_plan.hpp: prep_tile_body,
prep_elems_body, prep_clear_body), through pca_debug_prep_images -> prep_jobs_launch.  Bitwise against numpy.

The reference is the index formula of the kernel this launch replaced, restated: with perm32(p) = 4 g + j for
j < 4, else 16 + 4 g + j - 4 (g = p // 8, j = p % 8) and K(k) = (k & ~31) + perm32(k & 31),
    mode 0: dst[n cols + k] = src[n cols + k]          mode 1: dst[n cols + k] = src[n cols + K(k)]
    mode 2: dst[n rows + k] = src[K(k) cols + n]       mode 3: dst[n rows + k] = src[k cols + n]
on the FLAT source, rounded fp32 -> bf16 to nearest even by torch on the CPU.  Where K leaves the matrix (48 x 40:
columns 40 .. 51 of a row in mode 1, rows 48 .. 55 in mode 2) the formula reads on in the flat buffer, so every
source here stands in a backing buffer of 64 more rows than its shape, filled with the same seeded values; the
reference reads the same buffer.

Inputs: seeded normal values with +-0, the largest finite value, subnormals and round-to-even ties planted in
them.  NaN is left out: its payload is not the contract."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(32, 32), (128, 128), (256, 256), (128, 64), (48, 40), (128, 3)]
SPECIAL = np.array([0.0, -0.0, 3.4028234663852886e38, -3.4028234663852886e38, 1e-40, -1e-40, 1.4e-45, -1.4e-45,
                    1.1754942e-38, 1.00390625, 1.01171875, -1.00390625, 3.3895314e38, 65280.0, 9.1835e-41],
                   dtype=np.float32)
GUARD = 0x7B7B


def perm32(p):
    g, j = p >> 3, p & 7
    return np.where(j < 4, 4 * g + j, 16 + 4 * g + j - 4)


def K(k):
    return (k & ~31) + perm32(k & 31)


def source(rows, cols, seed):
    """Backing buffer [(rows + 64) cols]: the matrix is its first rows x cols elements."""
    rng = np.random.default_rng(seed)
    buf = rng.standard_normal((rows + 64) * cols).astype(np.float32)
    at = rng.choice(rows * cols, size=min(4 * len(SPECIAL), rows * cols // 2), replace=False)
    buf[at] = np.resize(SPECIAL, at.size)
    return buf


def reference(buf, rows, cols, mode):
    idx = np.arange(rows * cols)
    if mode <= 1:
        n, k = idx // cols, idx % cols
        at = n * cols + (K(k) if mode == 1 else k)
    else:
        n, k = idx // rows, idx % rows
        at = (K(k) if mode == 2 else k) * cols + n
    assert at.max() < buf.size
    return torch.from_numpy(buf[at]).to(torch.bfloat16).view(torch.int16).numpy()


def run(jobs):
    """jobs: (src tensor or None, dst tensor, rows, cols, mode); one launch."""
    from pca_hip import _lib
    n = len(jobs)
    src = (C.c_void_p * n)(*[0 if j[0] is None else j[0].data_ptr() for j in jobs])
    dst = (C.c_void_p * n)(*[j[1].data_ptr() for j in jobs])
    rows, cols, mode = ((C.c_int * n)(*[j[i] for j in jobs]) for i in (2, 3, 4))
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(_lib.lib().pca_debug_prep_images(src, dst, rows, cols, mode, n, st), "pca_debug_prep_images")
    torch.cuda.synchronize()


def image_buffer(dev, rows, cols):
    """dst with 64 guard words on either side."""
    return torch.full((rows * cols + 128,), GUARD, dtype=torch.int16, device=dev)


def judge(out, ref, what):
    got = out.cpu().numpy()
    assert (got[:64] == GUARD).all() and (got[-64:] == GUARD).all(), f"{what}: guard words written"
    bad = np.flatnonzero(got[64:-64] != ref)
    assert bad.size == 0, f"{what}: {bad.size} of {ref.size} words differ, first at {bad[:4]}"


@pytest.mark.parametrize("rows,cols", SHAPES)
def test_all_modes_of_one_source(rows, cols):
    """The four images of one source in one call: a group of three targets and a group of one (or, where the shape
    takes no tile, four element jobs)."""
    dev = torch.device("cuda", 0)
    buf = source(rows, cols, 4100 + rows + cols)
    s = torch.from_numpy(buf).to(dev)
    outs = [image_buffer(dev, rows, cols) for _ in range(4)]
    run([(s, outs[m][64:], rows, cols, m) for m in range(4)])
    for m in range(4):
        judge(outs[m], reference(buf, rows, cols, m), f"{rows} x {cols} mode {m}")


def test_three_targets_two_sources_and_a_misaligned_one():
    """A step-like table: three targets of one source, two of another, a target that is not 16-byte aligned (element
    items), and a clear - one launch."""
    dev = torch.device("cuda", 0)
    a, b = source(128, 128, 4301), source(128, 64, 4302)
    sa, sb = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
    jobs, want = [], []
    for src, buf, rows, cols, mode, shift in ((sa, a, 128, 128, 0, 0), (sb, b, 128, 64, 3, 0), (sa, a, 128, 128, 2, 0),
                                              (sa, a, 128, 128, 3, 0), (sb, b, 128, 64, 0, 0), (sa, a, 128, 128, 1, 3)):
        out = torch.full((rows * cols + 136,), GUARD, dtype=torch.int16, device=dev)
        jobs.append((src, out[64 + shift:], rows, cols, mode))
        want.append((out, shift, reference(buf, rows, cols, mode), f"{rows} x {cols} mode {mode} shift {shift}"))
    flags = torch.full((64 + 1000 + 64,), GUARD, dtype=torch.int16, device=dev)
    jobs.append((None, flags[64:], 1, 1000, 4))
    run(jobs)
    for out, shift, ref, what in want:
        got = out.cpu().numpy()
        assert (got[:64 + shift] == GUARD).all() and (got[64 + shift + ref.size:] == GUARD).all(), what
        assert (got[64 + shift:64 + shift + ref.size] == ref).all(), what
    got = flags.cpu().numpy()
    assert (got[:64] == GUARD).all() and (got[-64:] == GUARD).all() and (got[64:-64] == 0).all()


@pytest.mark.parametrize("shift", [0, 3, 13])
def test_clears_leave_the_guard_words(shift):
    """Clears of 1, 7, 8 and 4097 words, the range starting `shift` words past a 16-byte boundary: the words in front
    of it (the caller's, st_engine.hip: word 0 of the flag block) and behind it come back untouched."""
    dev = torch.device("cuda", 0)
    sizes = (1, 7, 8, 4097)
    bufs = [torch.full((64 + shift + n + 64,), GUARD, dtype=torch.int16, device=dev) for n in sizes]
    assert all(b.data_ptr() % 16 == 0 for b in bufs)
    run([(None, b[64 + shift:], 1, n, 4) for b, n in zip(bufs, sizes)])
    for b, n in zip(bufs, sizes):
        got = b.cpu().numpy()
        lo = 64 + shift
        assert (got[:lo] == GUARD).all(), (n, shift, "words in front of the range")
        assert (got[lo + n:] == GUARD).all(), (n, shift, "words behind the range")
        assert (got[lo:lo + n] == 0).all(), (n, shift)
