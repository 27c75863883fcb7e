"""Float64 numpy restatement of ``librosa.effects.trim`` (librosa 0.8 semantics; librosa itself is not
available, so this is "parity unpinned" like the resampler) and the seeded waveforms the trim tests
share.  A helper, not a test.

For a mono clip y of length L, frame_length (even) and hop_length:
  pad = frame_length // 2; ypad = reflect-pad of y by pad on both sides (needs L > pad)
  T = 1 + L // hop_length;  mse[t] = mean(ypad[t*hop : t*hop + frame_length] ** 2)
  db[t] = 10 log10(max(1e-10, mse[t])) - 10 log10(max(1e-10, max_t mse[t]))
  frame t is non-silent iff db[t] > -top_db (strict)
  (start, end) = (first * hop, min(L, (last + 1) * hop)) over the non-silent frames, (0, 0) without one.
"""
import numpy as np

AMIN = 1e-10


def frame_mse(y, frame_length=2048, hop_length=512):
    y = np.asarray(y, dtype=np.float64)
    pad = frame_length // 2
    assert frame_length % 2 == 0 and y.ndim == 1 and y.size > pad, (y.shape, frame_length)
    sq = np.pad(y, pad, mode="reflect") ** 2
    T = 1 + y.size // hop_length
    frames = np.lib.stride_tricks.sliding_window_view(sq, frame_length)[::hop_length][:T]
    assert frames.shape[0] == T
    return frames.mean(axis=1)


def frame_db(y, frame_length=2048, hop_length=512):
    mse = frame_mse(y, frame_length, hop_length)
    return 10.0 * np.log10(np.maximum(AMIN, mse)) - 10.0 * np.log10(max(AMIN, float(mse.max())))


def trim_ref(y, top_db=60, frame_length=2048, hop_length=512):
    """(start, end) of librosa.effects.trim(y, top_db, frame_length=, hop_length=)."""
    db = frame_db(y, frame_length, hop_length)
    keep = np.flatnonzero(db > -top_db)
    if keep.size == 0:
        return 0, 0
    return int(keep[0]) * hop_length, min(len(y), (int(keep[-1]) + 1) * hop_length)


def decision_margin(y, top_db=60, frame_length=2048, hop_length=512):
    """Smallest |db[t] + top_db| over the frames: how far the closest frame is from flipping."""
    return float(np.min(np.abs(frame_db(y, frame_length, hop_length) + top_db)))


# ---- the waveforms of tests/test_gpu_trim.py (checked for their margin in tests/test_trim_host.py) ----
CONFIGS = ((2048, 512), (1024, 256), (2048, 300))     # (frame_length, hop_length)
TOP_DBS = (20, 60)
FS = 44100
SWEEP_FS = 22050


def synth(clip_id, cls, n, fs=FS):
    """bench.py-style clip: 3 harmonics of 110 * 2^(cls/12) Hz with seeded phases + low-passed noise."""
    rng = np.random.Generator(np.random.PCG64(1000 + clip_id))
    t = np.arange(n) / fs
    f0 = 110.0 * 2.0 ** (cls / 12.0)
    x = np.zeros(n)
    for k in range(1, 4):
        x += (0.5 / k) * np.sin(2 * np.pi * f0 * k * t + rng.uniform(0, 2 * np.pi))
    x = x + 0.1 * np.convolve(rng.standard_normal(n), np.ones(8) / 8.0, mode="same")
    return (x / (np.max(np.abs(x)) + 1e-9) * 0.9).astype(np.float32)


def with_silence(x, lead, tail):
    return np.concatenate([np.zeros(lead, np.float32), x, np.zeros(tail, np.float32)])


def burst(seed, n, b0, b1, ramp, floor=1e-5, amp=0.5):
    """Gaussian noise of std ``floor`` with a burst of std ``amp`` over [b0, b1) that rises and falls
    linearly over ``ramp`` samples."""
    rng = np.random.Generator(np.random.PCG64(seed))
    k = np.arange(n)
    up = np.clip((k - b0) / ramp, 0, 1)
    down = np.clip((b1 - k) / ramp, 0, 1)
    env = floor + (amp - floor) * np.minimum(up, down)
    return (env * rng.standard_normal(n)).astype(np.float32)


def gpu_cases(frame_length, hop_length):
    """[(name, float32 waveform)] for one (frame_length, hop_length): every kind of clip the GPU test
    asks for.  38400 = lcm(512, 300) is a multiple of all three hops."""
    half = frame_length // 2
    tail_loud = np.zeros(5 * 38400 // 10 + 7, np.float32)
    tail_loud[-5:] = 0.5                                       # loud only in its last partial hop
    rng = np.random.Generator(np.random.PCG64(91))
    return [
        ("burst_ramp_a", burst(11, 50000, 12000, 30000, 4000)),
        ("burst_ramp_b", burst(12, 38400, 9000, 20000, 2500)),
        ("burst_ramp_c", burst(13, 61447, 30000, 52000, 6000, floor=3e-4)),
        ("synth_even", with_silence(synth(1, 3, 38400 - 7000 - 3100), 7000, 3100)),
        ("synth_odd", with_silence(synth(2, 7, 41000), 1234, 9321)),
        ("synth_lead_only", with_silence(synth(3, 0, 30001), 5555, 0)),
        ("half_plus_one", (0.3 * rng.standard_normal(half + 1)).astype(np.float32)),
        ("minute", burst(14, 60 * FS + 123, 700000, 1900000, 44100)),
        ("all_zero", np.zeros(20000, np.float32)),
        ("no_silence", synth(4, 5, 25000)),
        ("loud_tail", tail_loud),
    ]


def sweep_clips():
    """Clips (at SWEEP_FS) and labels of the end-to-end sweep checks: synthetic clips between digital
    silence of uneven length."""
    secs = (1.6, 1.1, 2.0, 0.9, 1.3)
    lead = (3000, 0, 8000, 1500, 5121)
    tail = (4100, 6000, 0, 2048, 777)
    clips = [with_silence(synth(70 + i, (3 * i) % 10, int(s * SWEEP_FS), SWEEP_FS), a, b)
             for i, (s, a, b) in enumerate(zip(secs, lead, tail))]
    return clips, [3, 1, 4, 1, 5]
