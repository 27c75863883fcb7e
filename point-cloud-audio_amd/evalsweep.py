"""Evaluation-time re-framing sweep on the device: the counterpart of the loop of
``Code/pceval.py:61-101`` (framewise model) for waveforms that are already decoded.

For every analysis length N the reference re-computes
``librosa.stft(x, n_fft=2**ceil(log2 N), win_length=N, hop_length=int(N*hf), window='hann') / N``
on the host, builds ``ESC_pc`` and runs the model over shuffled batches of 8, skipping the
short tail (``Code/pceval.py:76-97``).  Here the STFT, the point-set packing and the model all
run on the GPU; accuracy does not depend on the batch order, so batches are taken in order
and, as in the reference, an incomplete last batch is left out.

The sampling-rate axis (``for F in list_Fs``, ``librosa.resample(x, fsog, fs, 'kaiser_fast',
scale=True)``, ``Code/pceval.py:55,61,74``) runs on the device too: ``pca_hip.resample`` is a
band-limited sinc interpolation with resampy's documented ``kaiser_fast`` design.  librosa / resampy are
third-party, not vendored and not installed here, and the reference holds no resampled fixture, so this
axis is **parity unpinned** (SURVEY.md 8c); the kernel is checked against the CPU restatement of the
same algorithm (tests/test_resample.py).
The silence trim that precedes it (``x, index = librosa.effects.trim(x, top_db=trim_dB)``,
``Code/pceval.py:39,74``) runs on the device as well: the four re-framing sweeps take ``trim_dB`` (the
value a run's config file carries, ``trim_dB_of``) and trim every clip once, up front and before any
resampling, with ``pca_hip.trim_batch`` (librosa 0.8 semantics restated, default frame 2048 / hop 512;
**parity unpinned** for the same reason: checked against the numpy restatement tests/trim_ref.py).
``trim_dB=None`` (the default) leaves the clips as they are.
Not covered: ``librosa.load`` (file decoding is I/O: the clips passed in are waveforms already).

The other set-model experiments run here at batch scale too:

* ``subsample_sweep``: max-K / random-K sub-sampling, Code/pceval.py:107-192 (FST, per-frame point
  sets) and Code/pc_temp3d_eval.py:109-201 (3ST, per-chunk point sets);
* ``importance_sweep``: importance-sampled sets, Code/rebut_expts.py:55-149;
* ``attention_sweep``: sets reduced to the K points the model's own pooling attention weighs most
  (``STEngine.attention``, ``pca_hip.select_points``); no reference counterpart - a third curve beside
  random-K and max-K;
* ``reframe_sweep_temporal``: the (Fs, N) re-framing of the 3ST, Code/pc_temp3d_eval.py:56-107.
* ``clip_accuracy``: the clip-level scores the datasets' literature reports (majority vote and mean
  log-probability over a clip's frames or chunks, ``pca_hip.clip_aggregate``) next to the frame score;
  no reference counterpart - Code/pceval.py:95 scores frames.
* ``baseline_subsample_sweep``, ``baseline_reframe_sweep``, ``baseline_reframe_sweep_temporal``: the
  same experiments for the fixed-input baselines FB and CNN_temp (Code/baseline_eval.py,
  Code/baseline_temp_eval.py) on pca_hip.BaselineEngine, the selection fused into the forward launch.

Each K (or N) is one pass over the corpus: selection / packing launches write the point sets of many
of the reference's 8-set batches - and of all the random draws of that K - into one buffer, ONE
``STEngine.forward`` of up to a few hundred sets evaluates them, and ``pca_eval_tally`` adds the
correct predictions to device counters.  The host reads the counters once per K (or N), where the
reference syncs after every batch (``.item()``).  As in the reference, sets are taken in order and
only the first ``(n // batch_size) * batch_size`` count.
"""
import json
import math
from typing import Dict, Iterable, List, Optional, Sequence

import numpy as np
import torch

import ctypes as C

import pca_hip
from dataset import ESC_pc, ESC_pc_temp
from pca_hip import _lib
from pca_hip.baseline import SEL_ALL, BaselineEngine
from pca_hip.trainer import STEngine, st_config

__all__ = ["reframe_sweep", "framewise_dataset", "default_list_K", "sweep_draw", "subsample_sweep",
           "importance_sweep", "attention_sweep", "chunk_plan", "temporal_axes", "temporal_dataset",
           "reframe_sweep_temporal", "baseline_subsample_sweep", "baseline_frames",
           "baseline_chunks", "baseline_reframe_sweep", "baseline_reframe_sweep_temporal",
           "trim_dB_of", "trim_clips", "clip_accuracy"]


def trim_dB_of(config: Dict) -> Optional[float]:
    """The ``trim_dB`` of a run's config (``runfiles.load_run``; ``tDb = dict_params['trim_dB']``,
    Code/pceval.py:39) for the sweeps' ``trim_dB`` argument; None when the config has none."""
    v = config.get("trim_dB")
    return None if v is None else float(v)


def trim_clips(clips: Sequence[torch.Tensor], trim_dB: float, n_fft: int,
               ratios: Iterable[float] = (1.0,)) -> List[torch.Tensor]:
    """``librosa.effects.trim(x, top_db=trim_dB)`` of every clip (Code/pceval.py:74) in one
    pca_hip.trim_batch call; the results are views of ``clips``.  A clip whose trimmed length - at any
    of the resampling ``ratios`` (new rate / recorded rate) applied afterwards - is at or below the
    STFT's minimum n_fft / 2 raises ValueError: it would yield no spectrum, and the reference never
    drops a clip."""
    out, bounds = pca_hip.trim_batch(list(clips), top_db=trim_dB)
    need = int(n_fft) // 2
    for c, (s, e) in enumerate(bounds.tolist()):
        n = min(int(math.ceil((e - s) * float(r))) for r in ratios)
        if n <= need:
            raise ValueError(f"clip {c}: trim_dB={trim_dB:g} keeps samples [{s}, {e}) of "
                             f"{clips[c].numel()}, {n} samples for the STFT, which needs more than "
                             f"n_fft/2 = {need}")
    return out


def _pow2_fft(list_N) -> int:
    """The largest n_fft = 2**ceil(log2 N) of the set-model re-framing loops."""
    return max(1 << int(math.ceil(math.log2(n))) for n in list_N)


def framewise_dataset(clips: Sequence[torch.Tensor], labels: Sequence[int], fs: float, N: int,
                      hf: float = 0.5) -> ESC_pc:
    """ESC_pc over all frames of ``clips`` analysed with window length N
    (Code/pceval.py:74-83): n_fft = next power of two, hop = int(N*hf), all 1 + n_fft/2 bins,
    farr = linspace(0, fs/2, F) / fs.  Everything stays on the device."""
    n_fft = 1 << int(math.ceil(math.log2(N)))
    hop = int(N * hf)
    specs, labs = [], []
    for x, y in zip(clips, labels):
        s = pca_hip.stft_logmag(x, n_fft, win_length=N, hop=hop, frame_major=True)   # [T, F]
        specs.append(s)
        labs.append(torch.full((s.shape[0],), int(y), dtype=torch.int64, device=s.device))
    spec = torch.cat(specs, 0)
    F = spec.shape[1]
    farr = np.linspace(0, fs / 2, F) / fs
    return ESC_pc.from_device(spec, torch.cat(labs, 0), farr)


@torch.no_grad()
def reframe_sweep(model, clips: Sequence[torch.Tensor], labels: Sequence[int], fs: float,
                  list_N: Iterable[int], hf: float = 0.5, batch_size: int = 8,
                  mode: int = _lib.MODE_F32, json_file: Optional[str] = None,
                  list_Fs: Optional[Iterable[float]] = None,
                  trim_dB: Optional[float] = None) -> Dict:
    """Accuracy of ``model`` for every analysis length in ``list_N`` - and, with ``list_Fs``, for every
    sampling rate the clips (recorded at ``fs``) are resampled to first, as the double loop of
    ``Code/pceval.py:61-98`` does; returns (and optionally writes) the dictionary
    ``Code/pceval.py:57-59,99-104`` stores: ``{"data": {Fs: [acc per N]}, "list_Fs": [...],
    "list_N": [...]}``.  ``trim_dB``: trim every clip first (trim_clips; Code/pceval.py:74 trims, then
    resamples); None: the clips as given."""
    list_N = [int(n) for n in list_N]
    if list_Fs is not None:
        list_Fs = list(list_Fs)
    if trim_dB is not None:
        clips = trim_clips(clips, trim_dB, _pow2_fft(list_N),
                           (1.0,) if list_Fs is None else [F / fs for F in list_Fs])
    if list_Fs is not None:
        data = {}
        for F in list_Fs:
            rs = [pca_hip.resample(x, fs, F, scale=True) for x in clips]     # pceval.py:74
            data[F] = reframe_sweep(model, rs, labels, F, list_N, hf, batch_size, mode)["data"][F]
        out = {"data": data, "list_Fs": list_Fs, "list_N": list_N}
        if json_file is not None:
            with open(json_file, "w") as f:
                json.dump(out, f)
        return out
    accs: List[float] = []
    for N in list_N:
        ds = framewise_dataset(clips, labels, fs, N, hf)
        n = len(ds)
        full = (n // batch_size) * batch_size          # pceval.py:88-89 skips the short batch
        if full == 0:
            accs.append(float("nan"))
            continue
        # one engine launch covers many of the reference's 8-set batches
        chunk = batch_size * max(1, 256 // batch_size)
        dev = ds._resident()[0].device
        correct, done = 0, 0
        eng, eng_b = None, 0
        while done < full:
            b = min(chunk, full - done)
            if b != eng_b:
                eng, eng_b = STEngine(model, b, ds.num_points, mode, training=False), b
            X, lab = ds.batch(torch.arange(done, done + b, device=dev))
            correct += int((eng.forward(X).argmax(1) == lab).sum())
            done += b
        accs.append(correct / full)
    out = {"data": {fs: accs}, "list_Fs": [fs], "list_N": list_N}
    if json_file is not None:
        with open(json_file, "w") as f:
            json.dump(out, f)
    return out


# ---- batch-scale sweeps of the sub-sampling, importance and 3-D re-framing experiments ---------------
SETS_PER_CALL = 256            # sets per STEngine.forward when the caller does not say
WS_BUDGET = 4 << 30            # bytes of engine workspace one call may take (pca_st_ws_bytes)


def default_list_K(n: int) -> List[int]:
    """``np.arange(1, n, 50)`` with the last entry replaced by n: Code/pceval.py:111-112
    (n = Nfft // 2) and Code/pc_temp3d_eval.py:113-114, Code/rebut_expts.py:55-56
    (n = Nfft * Ntemp // 2)."""
    ks = np.arange(1, int(n), 50)
    if ks.size == 0:
        return [int(n)]
    ks[-1] = int(n)
    return [int(k) for k in ks]


def sweep_draw(step: int, run: int, n_runs: int) -> int:
    """Draw number of random run ``run`` of the ``step``-th K of a sweep (counted from 0 in loop
    order, across the winF loop of importance_sweep).  Every run of every K has its own, so runs
    differ; a selection is keyed by (seed, draw, batch slot, set index)."""
    return 1 + int(step) * int(n_runs) + int(run)


def _write_json(out: Dict, path: Optional[str]) -> None:
    if path is not None:
        with open(path, "w") as f:
            json.dump(out, f)


def _model_device(model) -> torch.device:
    return next(getattr(model, "module", model).parameters()).device


def _sets_per_call(model, npts: int, mode: int, want: Optional[int]) -> int:
    """Sets per engine call: ``want``, or SETS_PER_CALL halved until the inference workspace
    (pca_st_ws_bytes) fits WS_BUDGET."""
    if want is not None:
        assert want >= 1
        return int(want)
    cap = SETS_PER_CALL
    L = _lib.lib()
    while cap > 1:
        cfg = st_config(model, cap, npts, mode)
        if L.pca_st_ws_bytes(C.byref(cfg), 0) <= WS_BUDGET:
            break
        cap //= 2
    return cap


def _run_pieces(model, npts: int, din: int, mode: int, cap: int, pieces, select,
                counts: torch.Tensor) -> None:
    """Evaluate ``pieces`` = [(slot, draw, p0, p1)] (set positions p0 <= p < p1 selected with draw
    number ``draw``, their correct predictions tallied into counts[slot]) through engine calls of at
    most ``cap`` sets.  ``select(slot, draw, pos, out, labels_out)`` writes the point sets of the
    positions ``pos`` (device int64) into ``out`` [n, npts, din] and their labels into labels_out.
    Enqueues only: nothing here waits for the device."""
    calls, cur, fill = [], [], 0
    for slot, draw, p0, p1 in pieces:
        while p0 < p1:
            n = min(p1 - p0, cap - fill)
            cur.append((slot, draw, p0, p0 + n, fill))
            fill += n
            p0 += n
            if fill == cap:
                calls.append((cur, fill))
                cur, fill = [], 0
    if cur:
        calls.append((cur, fill))
    dev = counts.device
    engines = {}
    for parts, b in calls:
        if b not in engines:
            eng = STEngine(model, b, npts, mode, training=False)
            assert eng.cfg.k == 1, "sweeps score one prediction per set (PMA with one seed)"
            engines[b] = (eng, torch.empty((b, npts, din), dtype=torch.float32, device=dev),
                          torch.empty(b, dtype=torch.int64, device=dev))
        eng, X, lab = engines[b]
        for slot, draw, p0, p1, off in parts:
            pos = torch.arange(p0, p1, dtype=torch.int64, device=dev)
            select(slot, draw, pos, X[off:off + p1 - p0], lab[off:off + p1 - p0])
        logits = eng.forward(X)
        for slot, draw, p0, p1, off in parts:
            pca_hip.eval_tally(logits[off:off + p1 - p0], lab[off:off + p1 - p0], counts, slot)


def _resident_sets(spec, labels, farr, tarr, dev):
    """spec on ``dev`` in float32 with every set contiguous: [F, T] (FST frames) or [F, Nt, S]
    (3ST chunks) views; farr / tarr rounded to float32 once, as the datasets' .float() does."""
    x = torch.as_tensor(spec).to(dev, torch.float32)
    if tarr is None:
        assert x.dim() == 2, "FST: spec is [F, T]"
        x = x.t().contiguous().t()
    else:
        assert x.dim() == 3, "3ST: spec is [F, Nt, S]"
        x = x.permute(2, 1, 0).contiguous().permute(2, 1, 0)
    lab = torch.as_tensor(np.asarray(labels) if not torch.is_tensor(labels) else labels)
    lab = lab.to(dev, torch.int64).contiguous()
    f32 = torch.as_tensor(np.asarray(farr, dtype=np.float64)).float().to(dev)
    t32 = None if tarr is None else \
        torch.as_tensor(np.asarray(tarr, dtype=np.float64)).float().to(dev)
    return x, lab, f32, t32


def _two_pass_sweep(model, n_sets: int, npts_of_K, din: int, list_K, n_runs: int, batch_size: int,
                    mode: int, sets_per_call, select_of_K, step0: int = 0):
    """{K: [mean, var]} of the n_runs random runs and {K: [acc, 0]} of the deterministic pass (slot
    n_runs); one host read per K."""
    assert n_runs >= 1 and batch_size >= 1

    def run_K(K, pieces, counts):
        npts = npts_of_K(K)
        cap = _sets_per_call(model, npts, mode, sets_per_call)
        _run_pieces(model, npts, din, mode, cap, pieces, select_of_K(K), counts)

    return _k_passes((n_sets // batch_size) * batch_size, list_K, n_runs, _model_device(model),
                     run_K, step0)


def _k_passes(full: int, list_K, n_runs: int, dev, run_K, step0: int = 0):
    """The K loop of the two-pass sweeps: for every K, ``run_K(K, pieces, counts)`` evaluates the
    pieces [(slot, draw, 0, full)] - n_runs random runs, then the deterministic pass in slot n_runs
    - tallying into counts[slot]; one host read per K."""
    rand, det = {}, {}
    for ki, K in enumerate(list_K):
        if full == 0:
            rand[K], det[K] = [float("nan"), float("nan")], [float("nan"), 0]
            continue
        counts = torch.zeros(n_runs + 1, dtype=torch.int64, device=dev)
        pieces = [(r, sweep_draw(step0 + ki, r, n_runs), 0, full) for r in range(n_runs)]
        pieces.append((n_runs, 0, 0, full))
        run_K(K, pieces, counts)
        c = counts.tolist()                                    # the one host sync of this K
        accs = np.array([c[r] / full for r in range(n_runs)])
        rand[K] = [float(np.mean(accs)), float(np.var(accs))]
        det[K] = [c[n_runs] / full, 0]
    return rand, det


@torch.no_grad()
def subsample_sweep(model, spec, labels, farr, tarr=None, list_K: Optional[Iterable[int]] = None,
                    n_runs: int = 10, batch_size: int = 8, mode: int = _lib.MODE_F32,
                    seed: int = 0, json_files: Optional[Sequence[str]] = None,
                    sets_per_call: Optional[int] = None):
    """Experiment 2 of Code/pceval.py:107-192 (FST) and Code/pc_temp3d_eval.py:109-201 (3ST):
    accuracy of ``model`` on point sets reduced to K points, for every K in ``list_K``.

    FST: ``spec`` [F, T] frames (all 1 + Nfft/2 bins), ``tarr`` None; the points of a set are
    (farr[f], x) as utils.pc_randK / pc_maxK -> ESC_pc_ss build them.  Default list_K:
    default_list_K(F - 1) (n = Nfft // 2).
    3ST: ``spec`` [F, Nt, S] chunks, ``tarr`` [Nt]; points (farr[f], tarr[t], x) as
    ESC_pc_temp_randKSS / _maxKSS build them.  Default list_K: default_list_K(F * Nt).
    ``spec`` may be numpy or torch, host or device; ``labels`` int[T or S].

    For every K: ``n_runs`` random-K runs (mode 1; run r draws with number
    sweep_draw(index of K, r, n_runs) under ``seed``, batch slot = position of the set inside its
    selection launch) and one max-K pass (mode 0).  Max-K is exact: the K largest values of each
    set, as ``(-x).argsort()[:K]`` with equal values in ascending point order.  Random-K matches the
    reference in distribution only: the reference draws from the global numpy RNG, here the
    counter-based device stream draws.

    Returns (and, with ``json_files`` = (randK path, maxK path), writes) the two dictionaries of the
    reference: ``{"data": {K: [mean, var]}, "list_K": [...]}`` (np.var, ddof 0, over the runs) and
    ``{"data": {K: [acc, 0]}, "list_K": [...]}``."""
    dev = _model_device(model)
    x, lab, f32, t32 = _resident_sets(spec, labels, farr, tarr, dev)
    if tarr is None:
        F, n_sets = x.shape
        npts_all, din = F, 2
        default_n = F - 1
    else:
        F, Nt, n_sets = x.shape
        npts_all, din = F * Nt, 3
        default_n = F * Nt
    list_K = default_list_K(default_n) if list_K is None else [int(k) for k in list_K]
    assert all(1 <= k <= npts_all for k in list_K), (list_K, npts_all)

    def select_of_K(K):
        def select(slot, draw, pos, out, labels_out):
            m = pca_hip.MAXK if slot == n_runs else pca_hip.RANDK
            pca_hip.subsample_points(x, f32, t32, pos, K, m, seed, draw, lab, out=out,
                                     labels_out=labels_out)
        return select

    rand, det = _two_pass_sweep(model, n_sets, lambda K: K, din, list_K, n_runs, batch_size, mode,
                                sets_per_call, select_of_K)
    out_r = {"data": rand, "list_K": list_K}
    out_m = {"data": det, "list_K": list_K}
    if json_files is not None:
        _write_json(out_r, json_files[0])
        _write_json(out_m, json_files[1])
    return out_r, out_m


@torch.no_grad()
def importance_sweep(model, spec, labels, farr, tarr, list_K: Optional[Iterable[int]] = None,
                     list_winF: Iterable[int] = (64,), n_runs: int = 10, batch_size: int = 8,
                     mode: int = _lib.MODE_F32, seed: int = 0,
                     json_files: Optional[Sequence[str]] = None,
                     sets_per_call: Optional[int] = None):
    """The rebuttal experiment, Code/rebut_expts.py:55-149: accuracy of ``model`` on 3ST chunks
    (``spec`` [F, Nt, S], F >= 2, Nt >= 2) reduced to K importance-sampled points
    (ESC_pc_temp_importancerandKSS, pca_importance_points), for every smoothing width winF and K.

    ``choice`` 0 (K draws with replacement from the normalised heat map) runs ``n_runs`` times,
    run r of the i-th (winF, K) pair in loop order drawing with number sweep_draw(i, r, n_runs);
    it matches the reference in distribution only (the reference draws from torch's global
    generator).  ``choice`` 1 (the K hottest cells) runs once and is exact.

    Returns (and, with ``json_files`` = (randK path, maxK path), writes) the dictionaries of
    Code/rebut_expts.py:64-67, nested by winF: ``{"data": {winF: {K: [mean, var]}}, "list_K"}`` and
    ``{"data": {winF: {K: [acc, 0]}}, "list_K"}``.  Default list_K: default_list_K(F * Nt)."""
    dev = _model_device(model)
    x, lab, f32, t32 = _resident_sets(spec, labels, farr, tarr, dev)
    F, Nt, n_sets = x.shape
    list_K = default_list_K(F * Nt) if list_K is None else [int(k) for k in list_K]
    list_winF = [int(w) for w in list_winF]
    assert all(k >= 1 for k in list_K)
    rand, det = {}, {}
    for wi, winF in enumerate(list_winF):
        kern = pca_hip.importance_kernel(winF).to(dev)

        def select_of_K(K, kern=kern):
            def select(slot, draw, pos, out, labels_out):
                choice = 1 if slot == n_runs else 0
                pca_hip.importance_points(x, f32, t32, pos, K, choice, kern, seed, draw, lab,
                                          out=out, labels_out=labels_out)
            return select

        rand[winF], det[winF] = _two_pass_sweep(model, n_sets, lambda K: K, 3, list_K, n_runs,
                                                batch_size, mode, sets_per_call, select_of_K,
                                                step0=wi * len(list_K))
    out_r = {"data": rand, "list_K": list_K}
    out_m = {"data": det, "list_K": list_K}
    if json_files is not None:
        _write_json(out_r, json_files[0])
        _write_json(out_m, json_files[1])
    return out_r, out_m


def _pack_sets(x, f32, t32, pos, out):
    """The full point sets of the positions ``pos`` into ``out`` [n, N, din], as the datasets pack them:
    (farr[f], x) for FST frames, point p = t * F + f -> (farr[f], tarr[t], x) for 3ST chunks."""
    if t32 is None:
        pca_hip.pack_points_2d(x, f32, pos, out=out)
    else:
        pca_hip.pack_points_3d(x, f32, t32, pos, out=out)


@torch.no_grad()
def attention_sweep(model, spec, labels, farr, tarr=None, list_K: Optional[Iterable[int]] = None,
                    batch_size: int = 8, mode: int = _lib.MODE_F32, json_file: Optional[str] = None,
                    sets_per_call: Optional[int] = None):
    """Accuracy of ``model`` on point sets reduced to the K points its own pooling attention weighs most,
    for every K in ``list_K``.  **No reference counterpart**: the reference sub-samples by magnitude, at
    random (Code/pceval.py:107-192, Code/pc_temp3d_eval.py:109-201) or by a heat map of the input
    (Code/rebut_expts.py); this is the same experiment with the selection read off the trained model.

    Arguments and defaults as subsample_sweep: FST ``spec`` [F, T] frames with ``tarr`` None, 3ST ``spec``
    [F, Nt, S] chunks with ``tarr`` [Nt]; default list_K default_list_K(F - 1) / default_list_K(F * Nt).

    Pass 1 runs ``STEngine.attention`` over the sets that count (the first (n // batch_size) * batch_size)
    once, at full size, and keeps ``key`` - the mean of the pooling attention over seeds and heads,
    [n_sets, N] float32 - on the device.  Then, for every K, the sets are packed again piece by piece,
    reduced by ``pca_hip.select_points`` to the K points of largest key (descending; equal keys in
    ascending point order), evaluated by ``STEngine.forward`` at N = K and tallied by pca_eval_tally; one
    host read per K.  Engine calls hold up to ``sets_per_call`` sets (default: SETS_PER_CALL halved until
    the workspace fits WS_BUDGET, for the full-size pass and for every K).  The key is fp32 in every
    ``mode``; ``mode`` is the arithmetic of the forwards.

    Returns (and, with ``json_file``, writes) ``{"data": {K: [acc, 0]}, "list_K": [...]}``, the shape of the
    reference's max-K dictionary (paper_plots/FST_maxK_expt2.json), so the paper's plotting code can put
    the curve beside it."""
    dev = _model_device(model)
    x, lab, f32, t32 = _resident_sets(spec, labels, farr, tarr, dev)
    if tarr is None:
        F, n_sets = x.shape
        npts_all, din, default_n = F, 2, F - 1
    else:
        F, Nt, n_sets = x.shape
        npts_all, din, default_n = F * Nt, 3, F * Nt
    list_K = default_list_K(default_n) if list_K is None else [int(k) for k in list_K]
    assert all(1 <= k <= npts_all for k in list_K), (list_K, npts_all)
    full = (n_sets // batch_size) * batch_size
    data = {}
    if full == 0:
        data = {K: [float("nan"), 0] for K in list_K}
    else:
        # pass 1: the key of every set, resident
        key = torch.empty((full, npts_all), dtype=torch.float32, device=dev)
        cap = _sets_per_call(model, npts_all, mode, sets_per_call)
        engines = {}
        for p0 in range(0, full, cap):
            b = min(cap, full - p0)
            if b not in engines:
                eng = STEngine(model, b, npts_all, mode, training=False)
                assert eng.cfg.k == 1, "sweeps score one prediction per set (PMA with one seed)"
                engines[b] = (eng, torch.empty((b, npts_all, din), dtype=torch.float32, device=dev))
            eng, X = engines[b]
            _pack_sets(x, f32, t32, torch.arange(p0, p0 + b, dtype=torch.int64, device=dev), X)
            eng.attention(X, want_attn=False, key_out=key[p0:p0 + b])
        del engines
        full_buf = {}

        def select_of_K(K):
            def select(slot, draw, pos, out, labels_out):
                n = pos.numel()
                if n not in full_buf:          # the full-size sets of a piece and the indices kept
                    full_buf[n] = (torch.empty((n, npts_all, din), dtype=torch.float32, device=dev),
                                   torch.empty((n, K), dtype=torch.int32, device=dev))
                Xf, sel = full_buf[n]
                _pack_sets(x, f32, t32, pos, Xf)
                pca_hip.select_points(Xf, key.index_select(0, pos), K, out=out, sel=sel)
                torch.index_select(lab, 0, pos, out=labels_out)
            return select

        for K in list_K:
            counts = torch.zeros(1, dtype=torch.int64, device=dev)
            full_buf.clear()
            _run_pieces(model, K, din, mode, _sets_per_call(model, K, mode, sets_per_call),
                        [(0, 0, 0, full)], select_of_K(K), counts)
            data[K] = [int(counts.item()) / full, 0]           # the one host read of this K
    out = {"data": data, "list_K": list_K}
    _write_json(out, json_file)
    return out


def chunk_plan(frames: Sequence[int], Ntemp: int):
    """Where the Ntemp-frame chunks of a corpus lie when clip c's T_c = frames[c] STFT frames start at
    row frame_off[c] = the first multiple of Ntemp at or after the end of clip c - 1 (the layout of
    stft_logmag_batch(..., frame_align=Ntemp)).  Clip c yields T_c // Ntemp chunks, cut from its first
    frame with the short tail dropped, as ``np.hsplit(a, np.arange(0, T_c, Ntemp))`` minus the pieces
    narrower than Ntemp (Code/pc_temp3d_eval.py:78-83).  Chunk j covers rows j*Ntemp .. j*Ntemp +
    Ntemp - 1.  Returns (frame_off [n_clips + 1], chunk ids of the whole chunks in corpus order, the
    clip of each)."""
    foff, ids, clip_of = [0], [], []
    for c, t in enumerate(frames):
        j0 = foff[-1] // Ntemp
        for i in range(int(t) // Ntemp):
            ids.append(j0 + i)
            clip_of.append(c)
        foff.append(-(-(foff[-1] + int(t)) // Ntemp) * Ntemp)
    return foff, ids, clip_of


def temporal_axes(fs: float, N: int, Ntemp: int, hf: float = 0.5, F: Optional[int] = None):
    """(farr, tarr) of Code/pc_temp3d_eval.py:86-87 for analysis length N: farr = linspace(0, fs/2,
    F) / fs with F = n_fft / 2 bins (Nyquist dropped), tarr = linspace(0, (hf*N/fs)*Ntemp, Ntemp)."""
    if F is None:
        F = (1 << int(math.ceil(math.log2(N)))) // 2
    farr = np.linspace(0, fs / 2, F) / fs
    tarr = np.linspace(0, ((hf * N) / fs) * Ntemp, Ntemp)
    return farr, tarr


def temporal_dataset(clips: Sequence[torch.Tensor], labels: Sequence[int], fs: float, N: int,
                     Ntemp: int = 10, hf: float = 0.5):
    """(ESC_pc_temp over every Ntemp-frame chunk slot of the corpus, device int64 ids of the whole
    chunks in corpus order) for analysis length N (Code/pc_temp3d_eval.py:70-89): n_fft = 2**ceil(
    log2 N), win_length N, hop int(N*hf), Nyquist bin dropped, magnitude divided by N.  One STFT launch
    writes the clips frame-aligned (chunk_plan); the chunks are packed straight from it, so no
    spectrogram goes through the host."""
    n_fft = 1 << int(math.ceil(math.log2(N)))
    hop = int(N * hf)
    spec, foff = pca_hip.stft_logmag_batch(list(clips), n_fft, win_length=N, hop=hop,
                                           drop_nyquist=True, frame_major=True, norm=N,
                                           frame_align=Ntemp)
    frames = [int(pca_hip.lib().pca_stft_num_frames(int(x.numel()), hop)) for x in clips]
    plan_off, ids, clip_of = chunk_plan(frames, Ntemp)
    assert plan_off == foff, (plan_off, foff)
    F = n_fft // 2
    S = foff[-1] // Ntemp
    lab = np.full(S, -1, dtype=np.int64)
    lab[ids] = np.asarray([int(labels[c]) for c in clip_of], dtype=np.int64)
    dev = spec.device
    farr, tarr = temporal_axes(fs, N, Ntemp, hf, F)
    ds = ESC_pc_temp.from_device(spec.view(S, Ntemp, F), torch.as_tensor(lab).to(dev), farr, tarr)
    return ds, torch.as_tensor(np.asarray(ids, dtype=np.int64)).to(dev)


@torch.no_grad()
def reframe_sweep_temporal(model, clips: Sequence[torch.Tensor], labels: Sequence[int], fs: float,
                           list_N: Iterable[int], Ntemp: int = 10, hf: float = 0.5,
                           list_Fs: Optional[Iterable[float]] = None,
                           json_file: Optional[str] = None, batch_size: int = 8,
                           mode: int = _lib.MODE_F32, sets_per_call: Optional[int] = None,
                           trim_dB: Optional[float] = None) -> Dict:
    """Experiment 1 of Code/pc_temp3d_eval.py:56-107: accuracy of the 3ST ``model`` for every analysis
    length in ``list_N`` (temporal_dataset) and, with ``list_Fs``, every sampling rate the clips
    (recorded at ``fs``) are resampled to first (pca_hip.resample: parity unpinned, as in
    reframe_sweep).  Returns (and optionally writes) ``{"data": {Fs: [acc per N]}, "list_Fs": [...],
    "list_N": [...]}``; one host read per N.  ``trim_dB``: trim every clip first (trim_clips;
    Code/pc_temp3d_eval.py:73), before any resampling; None: the clips as given."""
    list_N = [int(n) for n in list_N]
    if list_Fs is not None:
        list_Fs = list(list_Fs)
    if trim_dB is not None:
        clips = trim_clips(clips, trim_dB, _pow2_fft(list_N),
                           (1.0,) if list_Fs is None else [F / fs for F in list_Fs])
    if list_Fs is not None:
        data = {}
        for F in list_Fs:
            rs = [pca_hip.resample(x, fs, F, scale=True) for x in clips]    # pc_temp3d_eval.py:74
            data[F] = reframe_sweep_temporal(model, rs, labels, F, list_N, Ntemp, hf,
                                             batch_size=batch_size, mode=mode,
                                             sets_per_call=sets_per_call)["data"][F]
        out = {"data": data, "list_Fs": list_Fs, "list_N": list_N}
        _write_json(out, json_file)
        return out
    dev = _model_device(model)
    accs: List[float] = []
    for N in list_N:
        ds, ids = temporal_dataset(clips, labels, fs, N, Ntemp, hf)
        full = (ids.numel() // batch_size) * batch_size   # pc_temp3d_eval.py:93-94: no short batch
        if full == 0:
            accs.append(float("nan"))
            continue
        npts = ds.num_points
        counts = torch.zeros(1, dtype=torch.int64, device=dev)

        def select(slot, draw, pos, out, labels_out):
            ds.batch(ids[pos], out=out, labels_out=labels_out)

        _run_pieces(model, npts, 3, mode, _sets_per_call(model, npts, mode, sets_per_call),
                    [(0, 0, 0, full)], select, counts)
        accs.append(int(counts.item()) / full)                # the one host sync of this N
    out = {"data": {fs: accs}, "list_Fs": [fs], "list_N": list_N}
    _write_json(out, json_file)
    return out


# ---- clip-level evaluation (no reference counterpart: Code/pceval.py:95 scores frames) ---------------
@torch.no_grad()
def clip_accuracy(model, clips: Sequence[torch.Tensor], labels: Sequence[int], fs: float, N: int,
                  Ntemp: Optional[int] = None, n_fft: Optional[int] = None,
                  trim_dB: Optional[float] = None, mode: int = _lib.MODE_F32,
                  batch_size: Optional[int] = None, json_file: Optional[str] = None,
                  hf: float = 0.5) -> Dict:
    """Frame-level and clip-level accuracy of ``model`` on ``clips`` analysed with window length N:
    every frame of every clip (framewise_dataset, an FST model) or, with ``Ntemp``, every whole
    Ntemp-frame chunk (temporal_dataset, a 3ST model) is one set, and a clip's prediction is taken
    over its sets by majority vote and by mean log-probability (pca_hip.clip_aggregate).

    Unlike the re-framing sweeps every set counts (a clip's score needs all of its sets, so no short
    batch is dropped).  The engine runs ``batch_size`` sets per call (default: SETS_PER_CALL, halved
    until the workspace fits WS_BUDGET) and its logits are kept in one device [n_sets, C] buffer;
    one clip_aggregate call and one pca_eval_tally call score it, and the host reads the three
    counters once, at the end - nothing waits for the device per batch.
    ``trim_dB``: trim every clip first (pca_hip.trim_batch: its read of the bounds is one more host
    read for the whole corpus, before any set is evaluated).  A clip that yields no set - n_fft / 2
    samples or fewer (after the trim), where the STFT has no frame to centre, or fewer than Ntemp
    frames - is counted in ``n_empty`` and left out of the clip scores, not refused.
    ``n_fft``: the datasets analyse with 2**ceil(log2 N); a value given must be that one.

    Returns (and optionally writes) ``{"frame", "clip_vote", "clip_mean", "n_sets", "n_clips",
    "n_empty"}``: correct sets / n_sets - what pca_eval_tally counts on the same logits - and correct
    clips / (n_clips - n_empty) under the two rules; NaN where the denominator is 0."""
    N = int(N)
    pow2 = _pow2_fft([N])
    if n_fft is not None and int(n_fft) != pow2:
        raise ValueError(f"n_fft={n_fft}: the datasets analyse N={N} with n_fft={pow2}")
    assert len(clips) == len(labels)
    clips = list(clips)
    if trim_dB is not None and clips:
        clips, _ = pca_hip.trim_batch(clips, top_db=trim_dB)
    hop = int(N * hf)
    L = _lib.lib()
    keep = [c for c, x in enumerate(clips) if int(x.numel()) > pow2 // 2]
    sets_of = [0] * len(clips)                     # sets per clip, in corpus order
    for c in keep:
        t = int(L.pca_stft_num_frames(int(clips[c].numel()), hop))
        sets_of[c] = t if Ntemp is None else t // int(Ntemp)
    n_sets, n_clips = sum(sets_of), len(clips)
    n_empty = sum(1 for n in sets_of if n == 0)
    nan = float("nan")
    out = {"frame": nan, "clip_vote": nan, "clip_mean": nan, "n_sets": n_sets, "n_clips": n_clips,
           "n_empty": n_empty}
    if n_sets == 0:
        _write_json(out, json_file)
        return out
    kept, klab = [clips[c] for c in keep], [int(labels[c]) for c in keep]
    if Ntemp is None:
        ds, ids, din = framewise_dataset(kept, klab, fs, N, hf), None, 2
        assert len(ds) == n_sets, (len(ds), n_sets)
    else:
        (ds, ids), din = temporal_dataset(kept, klab, fs, N, int(Ntemp), hf), 3
        assert ids.numel() == n_sets, (ids.numel(), n_sets)
    dev = _model_device(model)
    npts = ds.num_points
    cap = min(_sets_per_call(model, npts, mode, batch_size), n_sets)
    offs = np.concatenate([[0], np.cumsum(sets_of)]).astype(np.int64)
    offs_d = torch.as_tensor(offs).to(dev)
    clip_lab = torch.as_tensor(np.asarray([int(y) for y in labels], dtype=np.int64)).to(dev)
    set_lab = torch.empty(n_sets, dtype=torch.int64, device=dev)
    X = torch.empty((cap, npts, din), dtype=torch.float32, device=dev)
    logits, engines, done = None, {}, 0
    while done < n_sets:
        b = min(cap, n_sets - done)
        if b not in engines:
            engines[b] = STEngine(model, b, npts, mode, training=False)
            assert engines[b].cfg.k == 1, "one prediction per set (PMA with one seed)"
        eng = engines[b]
        if logits is None:
            logits = torch.empty((n_sets, eng.cfg.C), dtype=torch.float32, device=dev)
        pos = torch.arange(done, done + b, dtype=torch.int64, device=dev)
        ds.batch(pos if ids is None else ids[pos], out=X[:b], labels_out=set_lab[done:done + b])
        logits[done:done + b].copy_(eng.forward(X[:b]))
        done += b
    counts = torch.zeros(3, dtype=torch.int64, device=dev)
    pca_hip.clip_aggregate(logits, offs_d, clip_lab, counts, 0)      # counts[0], counts[1]
    pca_hip.eval_tally(logits, set_lab, counts, 2)
    vote, mean, frame = counts.tolist()                               # the one host read
    out["frame"] = frame / n_sets
    out["clip_vote"] = vote / (n_clips - n_empty)
    out["clip_mean"] = mean / (n_clips - n_empty)
    _write_json(out, json_file)
    return out


# ---- the fixed-input baselines (FB, CNN_temp): Code/baseline_eval.py, Code/baseline_temp_eval.py ------
# The same passes as above on BaselineEngine (pca_fb_forward / pca_cnn_temp_forward): the selection
# happens inside the forward launch, which reads the sets in place, so one launch per run and K
# covers up to BASELINE_SETS_PER_CALL sets.  The counting follows the reference scripts: FB counts
# every frame (batch 128, no batch skipped, Code/baseline_eval.py:84-90,148-157); CNN_temp runs
# batches of 2 and skips a trailing one-set batch (Code/baseline_temp_eval.py:43,95-96,152-153).
BASELINE_SETS_PER_CALL = 16384
FB_BATCH, CNN_TEMP_BATCH = 128, 2


def _baseline_engine(model) -> BaselineEngine:
    return model if isinstance(model, BaselineEngine) else BaselineEngine(model)


def _baseline_full(eng: BaselineEngine, n_sets: int) -> int:
    """Sets that count: all (FB), all but a trailing one-set batch (CNN_temp)."""
    return (n_sets // CNN_TEMP_BATCH) * CNN_TEMP_BATCH if eng.cnn else n_sets


def _baseline_run(eng: BaselineEngine, x, lab, ids, pieces, counts, K=None, sel_of_slot=None,
                  seed: int = 0, cap: Optional[int] = None) -> None:
    """Forward + tally of ``pieces`` = [(slot, draw, p0, p1)]: the sets ids[p0:p1] (ids None: the
    positions themselves), cell selection ``sel_of_slot(slot)`` (default: none), in launches of at
    most ``cap`` sets.  Enqueues only."""
    cap = BASELINE_SETS_PER_CALL if cap is None else int(cap)
    dev = counts.device
    n_max = min(cap, max(p1 - p0 for _, _, p0, p1 in pieces))
    out = torch.empty((n_max, eng.nclasses), dtype=torch.float32, device=dev)
    lab_out = torch.empty(n_max, dtype=torch.int64, device=dev)
    for slot, draw, p0, p1 in pieces:
        for a in range(p0, p1, cap):
            b = min(a + cap, p1)
            idx = torch.arange(a, b, dtype=torch.int64, device=dev) if ids is None else ids[a:b]
            mode = SEL_ALL if sel_of_slot is None else sel_of_slot(slot)
            o, lo = out[:b - a], lab_out[:b - a]
            eng.forward(x, idx, K, mode, seed, draw, labels=lab, out=o, labels_out=lo)
            pca_hip.eval_tally(o, lo, counts, slot)


@torch.no_grad()
def baseline_subsample_sweep(model, spec, labels, list_K: Optional[Iterable[int]] = None,
                             n_runs: int = 10, seed: int = 0,
                             json_files: Optional[Sequence[str]] = None,
                             sets_per_call: Optional[int] = None):
    """Experiment 2 of Code/baseline_eval.py:111-200 (FB) and Code/baseline_temp_eval.py:110-200
    (CNN_temp): accuracy of the baseline ``model`` (baseline_ff / CNN_classifier or a BaselineEngine)
    on inputs with all but K cells zeroed, for every K in ``list_K``.

    FB: ``spec`` [F, T] frames (F = layer_dims[0]); the frame's other bins are zeroed as by
    pc_randK_replace / pc_maxK_replace.  Default list_K: default_list_K(F - 1) (Nfft // 2).
    CNN_temp: ``spec`` [F, Nt, S] chunks; the chunk's other cells are zeroed as by
    ESC_baseline_temporal_maxK(flag "rand" / "max") over the cells p = t*F + f.  Default list_K:
    default_list_K(F * Nt).  ``spec`` may be numpy or torch, host or device; ``labels`` int[T or S].

    For every K: ``n_runs`` random-K runs (run r draws with number sweep_draw(index of K, r, n_runs)
    under ``seed``, batch slot = position of the set inside its launch) and one max-K pass.  Max-K
    keeps the cells pca_subsample_points keeps (equal values in ascending cell order, NaN last) and
    is exact; random-K matches the reference in distribution only.  Returns (and, with
    ``json_files`` = (randK path, maxK path), writes) ``{"data": {K: [mean, var]}, "list_K"}`` and
    ``{"data": {K: [acc, 0]}, "list_K"}``, the layout of paper_plots/{FB,CNNTemp}_{randK,maxK}_expt2.json."""
    eng = _baseline_engine(model)
    x = torch.as_tensor(spec).to(eng.dev, torch.float32)
    if eng.cnn:
        assert x.dim() == 3, "CNN_temp: spec is [F, Nt, S]"
        x = x.permute(2, 1, 0).contiguous().permute(2, 1, 0)
    else:
        assert x.dim() == 2, "FB: spec is [F, T]"
        x = x.t().contiguous().t()
    lab = torch.as_tensor(np.asarray(labels) if not torch.is_tensor(labels) else labels)
    lab = lab.to(eng.dev, torch.int64).contiguous()
    n_cells = x.shape[0] * (x.shape[1] if eng.cnn else 1)
    n_sets = x.shape[-1]
    list_K = default_list_K(n_cells if eng.cnn else n_cells - 1) if list_K is None \
        else [int(k) for k in list_K]
    assert all(1 <= k <= n_cells for k in list_K), (list_K, n_cells)

    def run_K(K, pieces, counts):
        _baseline_run(eng, x, lab, None, pieces, counts, K,
                      lambda slot: pca_hip.MAXK if slot == n_runs else pca_hip.RANDK, seed,
                      sets_per_call)

    rand, det = _k_passes(_baseline_full(eng, n_sets), list_K, n_runs, eng.dev, run_K)
    out_r = {"data": rand, "list_K": list_K}
    out_m = {"data": det, "list_K": list_K}
    if json_files is not None:
        _write_json(out_r, json_files[0])
        _write_json(out_m, json_files[1])
    return out_r, out_m


def baseline_frames(clips: Sequence[torch.Tensor], labels: Sequence[int], N: int, n_fft: int,
                    hf: float = 0.5):
    """(spec [F, T] device view, labels int64 [T]) of every frame of ``clips`` for FB's Experiment 1
    (Code/baseline_eval.py:71-81): librosa.stft(x, n_fft, win_length=N, hop=int(N*hf), 'hann') /
    n_fft, log(1e-8 + |.|), all 1 + n_fft/2 bins.  n_fft stays the model's window whatever N is:
    the input width is fixed."""
    assert 1 <= N <= n_fft
    spec, foff = pca_hip.stft_logmag_batch(list(clips), n_fft, win_length=N, hop=int(N * hf),
                                           frame_major=True)              # [T, F]
    dev = spec.device
    lab = torch.cat([torch.full((foff[c + 1] - foff[c],), int(y), dtype=torch.int64, device=dev)
                     for c, y in enumerate(labels)])
    return spec.t(), lab


def baseline_chunks(clips: Sequence[torch.Tensor], labels: Sequence[int], N: int, n_fft: int,
                    Ntemp: int = 10, hf: float = 0.5):
    """(spec [F, Ntemp, S] device view over every Ntemp-frame chunk slot, labels int64 [S], ids of
    the whole chunks in corpus order) for CNN_temp's Experiment 1 (Code/baseline_temp_eval.py:
    78-91): librosa.stft(x, n_fft, win_length=N, hop=int(N*hf)) / n_fft, Nyquist bin dropped,
    log(1e-8 + |.|), chunks of Ntemp frames cut from each clip's first frame, short tail dropped
    (chunk_plan).  n_fft stays the model's window whatever N is."""
    assert 1 <= N <= n_fft
    hop = int(N * hf)
    spec, foff = pca_hip.stft_logmag_batch(list(clips), n_fft, win_length=N, hop=hop,
                                           drop_nyquist=True, frame_major=True,
                                           frame_align=Ntemp)
    frames = [int(pca_hip.lib().pca_stft_num_frames(int(x.numel()), hop)) for x in clips]
    plan_off, ids, clip_of = chunk_plan(frames, Ntemp)
    assert plan_off == foff, (plan_off, foff)
    F = n_fft // 2
    S = foff[-1] // Ntemp
    lab = np.full(S, -1, dtype=np.int64)
    lab[ids] = np.asarray([int(labels[c]) for c in clip_of], dtype=np.int64)
    dev = spec.device
    return (spec.view(S, Ntemp, F).permute(2, 1, 0), torch.as_tensor(lab).to(dev),
            torch.as_tensor(np.asarray(ids, dtype=np.int64)).to(dev))


@torch.no_grad()
def _baseline_reframe(model, clips, labels, fs, list_N, hf, list_Fs, json_file, n_fft, Ntemp,
                      sets_per_call, trim_dB=None):
    eng = _baseline_engine(model)
    list_N = [int(n) for n in list_N]
    if n_fft is None:
        n_fft = 2 * eng.Nf if eng.cnn else 2 * (eng.layer_dims[0] - 1)
    if list_Fs is not None:
        list_Fs = list(list_Fs)
    if trim_dB is not None:                      # Code/baseline_eval.py:74: trim, then resample
        clips = trim_clips(clips, trim_dB, n_fft,
                           (1.0,) if list_Fs is None else [F / fs for F in list_Fs])
    if list_Fs is not None:
        data = {}
        for F in list_Fs:
            rs = [pca_hip.resample(x, fs, F, scale=True) for x in clips]
            data[F] = _baseline_reframe(eng, rs, labels, F, list_N, hf, None, None, n_fft, Ntemp,
                                        sets_per_call)["data"][F]
        out = {"data": data, "list_Fs": list_Fs, "list_N": list_N}
        _write_json(out, json_file)
        return out
    accs: List[float] = []
    for N in list_N:
        if eng.cnn:
            x, lab, ids = baseline_chunks(clips, labels, N, n_fft, Ntemp, hf)
            n_sets = ids.numel()
        else:
            x, lab = baseline_frames(clips, labels, N, n_fft, hf)
            ids, n_sets = None, x.shape[1]
        full = _baseline_full(eng, n_sets)
        if full == 0:
            accs.append(float("nan"))
            continue
        counts = torch.zeros(1, dtype=torch.int64, device=eng.dev)
        _baseline_run(eng, x, lab, ids, [(0, 0, 0, full)], counts, cap=sets_per_call)
        accs.append(int(counts.item()) / full)                # the one host sync of this N
    out = {"data": {fs: accs}, "list_Fs": [fs], "list_N": list_N}
    _write_json(out, json_file)
    return out


def baseline_reframe_sweep(model, clips: Sequence[torch.Tensor], labels: Sequence[int], fs: float,
                           list_N: Iterable[int], hf: float = 0.5,
                           list_Fs: Optional[Iterable[float]] = None,
                           json_file: Optional[str] = None, n_fft: Optional[int] = None,
                           sets_per_call: Optional[int] = None,
                           trim_dB: Optional[float] = None) -> Dict:
    """Experiment 1 of Code/baseline_eval.py:50-103 (FB): accuracy for every analysis length N in
    ``list_N`` (baseline_frames: n_fft = the model's window 2 * (layer_dims[0] - 1) unless given,
    divisor n_fft, every frame counts) and, with ``list_Fs``, every sampling rate the clips
    (recorded at ``fs``) are resampled to first (pca_hip.resample: parity unpinned).  Returns (and
    optionally writes) ``{"data": {Fs: [acc per N]}, "list_Fs", "list_N"}`` (FB_expt1.json).
    ``trim_dB``: trim every clip first (trim_clips; Code/baseline_eval.py:74); None: as given."""
    eng = _baseline_engine(model)
    assert not eng.cnn, "baseline_reframe_sweep takes an FB model (CNN_temp: _temporal)"
    return _baseline_reframe(eng, clips, labels, fs, list_N, hf, list_Fs, json_file, n_fft, None,
                             sets_per_call, trim_dB)


def baseline_reframe_sweep_temporal(model, clips: Sequence[torch.Tensor], labels: Sequence[int],
                                    fs: float, list_N: Iterable[int], hf: float = 0.5,
                                    list_Fs: Optional[Iterable[float]] = None,
                                    json_file: Optional[str] = None, n_fft: Optional[int] = None,
                                    sets_per_call: Optional[int] = None,
                                    trim_dB: Optional[float] = None) -> Dict:
    """Experiment 1 of Code/baseline_temp_eval.py:51-107 (CNN_temp): as baseline_reframe_sweep on
    the model's Nt-frame chunks (baseline_chunks: n_fft = 2 * Nf unless given, Nyquist dropped,
    divisor n_fft, short tail dropped, a trailing one-set batch of 2 skipped).  Writes the layout of
    CNNTemp_expt1.json.  ``trim_dB``: as in baseline_reframe_sweep (Code/baseline_temp_eval.py:72)."""
    eng = _baseline_engine(model)
    assert eng.cnn, "baseline_reframe_sweep_temporal takes a CNN_temp model"
    return _baseline_reframe(eng, clips, labels, fs, list_N, hf, list_Fs, json_file, n_fft, eng.Nt,
                             sets_per_call, trim_dB)
