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
* ``peak_sweep``: sets reduced to their K strongest spectral peaks, refined off the grid
  (``pca_hip.peak_points``), evaluated as padded sets with their point counts; no reference counterpart
  - a fourth curve;
* ``reassign_sweep``: sets whose points slide from the grid to their reassigned time-frequency coordinates
  (``pca_hip.frame_points_reassigned``), one pass per strength; no reference counterpart;
* ``multires_sweep``: sets that hold several STFT resolutions at once (``pca_hip.frame_points_multires``),
  scored with all levels and with subsets of them, one pass per subset; no reference counterpart;
* ``band_sweep``: log-mel / filter-bank point sets (``pca_hip.frame_points_bands``) at several band counts,
  one pass per bank over one resident corpus; no reference counterpart;
* ``pcen_sweep``: band point sets with per-channel energy normalisation (``pca_hip.frame_points_pcen``) for
  several ``Pcen`` specs beside the log-band column, one pass each; no reference counterpart;
* ``delta_sweep``: grid or band point sets with delta columns (``pca_hip.frame_points_delta``) at several
  regression widths, one pass each; no reference counterpart;
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

How the sweeps are put together - a new experiment is one more caller of these, not one more copy:

* ``_reframe_driver``: the (Fs, N) loop of the four re-framing sweeps - trim once, resample once per
  rate, ``acc_of_N`` per N, the dictionary and its JSON; a sweep supplies ``acc_of_N`` only;
* ``_run_pieces``: the engine pass of every set-model sweep, ``reframe_sweep`` included (call packing,
  selection, forward, tally), on engines from ``_engine_cache`` (one ``STEngine`` and its buffers
  per call size; also pass 1 of ``attention_sweep`` and ``clip_accuracy``); ``_dataset_accuracy`` is
  one such pass over a dataset, NaN for an empty one; ``_baseline_run`` is the BaselineEngine
  counterpart of ``_run_pieces``;
* ``_k_passes`` / ``_two_pass_sweep``: the K loop of random runs plus one deterministic pass;
* ``_set_contiguous`` (within ``_resident_sets``), ``_set_geometry``, ``_norm_list_K``,
  ``_chunk_labels``, ``_two_dicts``: the set layout, its sizes, the K grid, the chunk labels and the
  two-dictionary return that the set-model sweeps and the baselines share.
"""
import json
import math
from typing import Dict, Iterable, List, Optional, Sequence

import numpy as np
import torch

import ctypes as C

import pca_hip
from dataset import ESC_pc, ESC_pc_temp, ESC_wave_pc, ESC_wave_pc_multires, ESC_wave_pc_temp
from pca_hip import _lib
from pca_hip.baseline import SEL_ALL, BaselineEngine
from pca_hip.trainer import STEngine, st_config

__all__ = ["reframe_sweep", "framewise_dataset", "default_list_K", "sweep_draw", "subsample_sweep",
           "importance_sweep", "attention_sweep", "peak_sweep", "most_peaks", "reassign_sweep", "multires_sweep",
           "band_sweep", "pcen_sweep", "delta_sweep",
           "default_level_subsets", "chunk_plan",
           "temporal_axes", "temporal_dataset", "reframe_sweep_temporal", "baseline_subsample_sweep", "baseline_frames",
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


def _write_json(out: Dict, path: Optional[str]) -> None:
    if path is not None:
        with open(path, "w") as f:
            json.dump(out, f)


def _reframe_driver(clips, labels, fs, list_N, list_Fs, trim_dB, trim_n_fft, json_file,
                    acc_of_N) -> Dict:
    """The (Fs, N) double loop of the re-framing sweeps (Code/pceval.py:61-104 and its counterparts):
    trims every clip once, before any resampling, checked against ``trim_n_fft`` (None: the set
    models' _pow2_fft(list_N)) at the ratios F / fs; resamples once per rate of ``list_Fs`` (None: the
    clips as recorded, at ``fs``); ``acc_of_N(clips_at_rate, rate, N) -> float`` gives each entry.
    Returns and writes ``{"data": {Fs: [acc per N]}, "list_Fs": [...], "list_N": [...]}``."""
    list_N = [int(n) for n in list_N]
    rates = None if list_Fs is None else list(list_Fs)
    if trim_dB is not None:
        clips = trim_clips(clips, trim_dB, _pow2_fft(list_N) if trim_n_fft is None else trim_n_fft,
                           (1.0,) if rates is None else [F / fs for F in rates])
    data = {}
    for F in [fs] if rates is None else rates:
        at_rate = clips if rates is None else \
            [pca_hip.resample(x, fs, F, scale=True) for x in clips]      # pceval.py:74
        data[F] = [acc_of_N(at_rate, F, N) for N in list_N]
    out = {"data": data, "list_Fs": [fs] if rates is None else rates, "list_N": list_N}
    _write_json(out, json_file)
    return out


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
    resamples); None: the clips as given.  One engine call covers many of the reference's 8-set
    batches (batch_size * max(1, 256 // batch_size) sets) and the host reads the count once per N;
    like every sweep on _run_pieces it takes a model with one prediction per set (PMA, one seed)."""
    def acc_of_N(at_rate, F, N):
        # pceval.py:88-89 skips the short batch; the call size is fixed, not the workspace rule
        return _dataset_accuracy(model, framewise_dataset(at_rate, labels, F, N, hf), None, 2,
                                 batch_size, mode, batch_size * max(1, 256 // batch_size))

    return _reframe_driver(clips, labels, fs, list_N, list_Fs, trim_dB, None, json_file, acc_of_N)


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


def _engine_cache(model, npts: int, mode: int, dev, *bufs):
    """get(b) -> [STEngine(model, b, npts, mode, training=False), one tensor [b, *shape] of ``dtype``
    on ``dev`` per (shape, dtype) of ``bufs``], built once per call size b, on its first use."""
    cache = {}

    def get(b):
        if b not in cache:
            eng = STEngine(model, b, npts, mode, training=False)
            assert eng.cfg.k == 1, "sweeps score one prediction per set (PMA with one seed)"
            cache[b] = [eng] + [torch.empty((b, *shape), dtype=dtype, device=dev)
                                for shape, dtype in bufs]
        return cache[b]
    return get


def _run_pieces(model, npts: int, din: int, mode: int, cap: int, pieces, select,
                counts: torch.Tensor, with_lengths: bool = False) -> None:
    """Evaluate ``pieces`` = [(slot, draw, p0, p1)] (set positions p0 <= p < p1 selected with draw
    number ``draw``, their correct predictions tallied into counts[slot]) through engine calls of at
    most ``cap`` sets.  ``select(slot, draw, pos, out, labels_out)`` writes the point sets of the
    positions ``pos`` (device int64) into ``out`` [n, npts, din] and their labels into labels_out.
    ``with_lengths``: every call also has an int32 buffer of point counts; ``select`` takes its slice as a
    sixth argument, ``lengths_out``, and fills it, and the forward reads it (padded sets).
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
    bufs = [((npts, din), torch.float32), ((), torch.int64)] + ([((), torch.int32)] if with_lengths else [])
    engines = _engine_cache(model, npts, mode, dev, *bufs)
    for parts, b in calls:
        eng, X, lab, *ln = engines(b)
        for slot, draw, p0, p1, off in parts:
            pos = torch.arange(p0, p1, dtype=torch.int64, device=dev)
            select(slot, draw, pos, X[off:off + p1 - p0], lab[off:off + p1 - p0],
                   *(t[off:off + p1 - p0] for t in ln))
        logits = eng.forward(X, *ln)
        for slot, draw, p0, p1, off in parts:
            pca_hip.eval_tally(logits[off:off + p1 - p0], lab[off:off + p1 - p0], counts, slot)


def _dataset_accuracy(model, ds, ids, din: int, batch_size: int, mode: int, sets_per_call) -> float:
    """Accuracy of ``model`` over the first (n // batch_size) * batch_size sets of ``ds`` - of the
    sets ``ids`` (device int64) when given - in one _run_pieces pass of calls of _sets_per_call(...,
    ``sets_per_call``) sets and one host read; NaN when there is no full batch."""
    full = ((len(ds) if ids is None else ids.numel()) // batch_size) * batch_size
    if full == 0:
        return float("nan")
    counts = torch.zeros(1, dtype=torch.int64, device=_model_device(model))

    def select(slot, draw, pos, out, labels_out):
        ds.batch(pos if ids is None else ids[pos], out=out, labels_out=labels_out)

    npts = ds.num_points
    _run_pieces(model, npts, din, mode, _sets_per_call(model, npts, mode, sets_per_call),
                [(0, 0, 0, full)], select, counts)
    return int(counts.item()) / full                              # the one host sync of this pass


def _set_contiguous(spec, labels, dev, temporal: bool):
    """(spec on ``dev`` in float32 with every set contiguous - an [F, T] view of frames, or with
    ``temporal`` an [F, Nt, S] view of chunks -, labels int64 on ``dev``)."""
    x = torch.as_tensor(spec).to(dev, torch.float32)
    if temporal:
        assert x.dim() == 3, "chunks (3ST, CNN_temp): spec is [F, Nt, S]"
        x = x.permute(2, 1, 0).contiguous().permute(2, 1, 0)
    else:
        assert x.dim() == 2, "frames (FST, FB): spec is [F, T]"
        x = x.t().contiguous().t()
    lab = torch.as_tensor(np.asarray(labels) if not torch.is_tensor(labels) else labels)
    return x, lab.to(dev, torch.int64).contiguous()


def _resident_sets(spec, labels, farr, tarr, dev):
    """spec on ``dev`` in float32 with every set contiguous: [F, T] (FST frames) or [F, Nt, S]
    (3ST chunks) views; farr / tarr rounded to float32 once, as the datasets' .float() does."""
    x, lab = _set_contiguous(spec, labels, dev, tarr is not None)
    f32 = torch.as_tensor(np.asarray(farr, dtype=np.float64)).float().to(dev)
    t32 = None if tarr is None else \
        torch.as_tensor(np.asarray(tarr, dtype=np.float64)).float().to(dev)
    return x, lab, f32, t32


def _set_geometry(x: torch.Tensor, temporal: bool):
    """(n_sets, points or cells per set, din of the packed points, n of the default K grid
    default_list_K(n)) of a _set_contiguous spec: frames [F, T] -> (T, F, 2, F - 1 = Nfft // 2),
    chunks [F, Nt, S] -> (S, F * Nt, 3, F * Nt)."""
    if not temporal:
        F, n_sets = x.shape
        return n_sets, F, 2, F - 1
    F, Nt, n_sets = x.shape
    return n_sets, F * Nt, 3, F * Nt


def _norm_list_K(list_K, default_n: int, k_max: Optional[int] = None) -> List[int]:
    """``list_K`` as ints (None: default_list_K(default_n)), every K at least 1 and, where given, at
    most ``k_max``."""
    list_K = default_list_K(default_n) if list_K is None else [int(k) for k in list_K]
    assert all(k >= 1 and (k_max is None or k <= k_max) for k in list_K), (list_K, k_max)
    return list_K


def _two_dicts(rand, det, list_K, json_files):
    """The two dictionaries of the K sweeps, ``{"data": rand, "list_K"}`` and ``{"data": det,
    "list_K"}``, written to ``json_files`` = (randK path, maxK path) when given."""
    out_r = {"data": rand, "list_K": list_K}
    out_m = {"data": det, "list_K": list_K}
    if json_files is not None:
        _write_json(out_r, json_files[0])
        _write_json(out_m, json_files[1])
    return out_r, out_m


def _two_pass_sweep(model, n_sets: int, din: int, list_K, n_runs: int, batch_size: int,
                    mode: int, sets_per_call, select_of_K, step0: int = 0):
    """{K: [mean, var]} of the n_runs random runs and {K: [acc, 0]} of the deterministic pass (slot
    n_runs) on sets of K points; one host read per K."""
    assert n_runs >= 1 and batch_size >= 1

    def run_K(K, pieces, counts):
        cap = _sets_per_call(model, K, mode, sets_per_call)
        _run_pieces(model, K, din, mode, cap, pieces, select_of_K(K), counts)

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
    n_sets, npts_all, din, default_n = _set_geometry(x, tarr is not None)
    list_K = _norm_list_K(list_K, default_n, npts_all)

    def select_of_K(K):
        def select(slot, draw, pos, out, labels_out):
            m = pca_hip.MAXK if slot == n_runs else pca_hip.RANDK
            pca_hip.subsample_points(x, f32, t32, pos, K, m, seed, draw, lab, out=out,
                                     labels_out=labels_out)
        return select

    rand, det = _two_pass_sweep(model, n_sets, din, list_K, n_runs, batch_size, mode,
                                sets_per_call, select_of_K)
    return _two_dicts(rand, det, list_K, json_files)


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
    n_sets, _, din, default_n = _set_geometry(x, True)
    list_K = _norm_list_K(list_K, default_n)
    list_winF = [int(w) for w in list_winF]
    rand, det = {}, {}
    for wi, winF in enumerate(list_winF):
        kern = pca_hip.importance_kernel(winF).to(dev)

        def select_of_K(K, kern=kern):
            def select(slot, draw, pos, out, labels_out):
                choice = 1 if slot == n_runs else 0
                pca_hip.importance_points(x, f32, t32, pos, K, choice, kern, seed, draw, lab,
                                          out=out, labels_out=labels_out)
            return select

        rand[winF], det[winF] = _two_pass_sweep(model, n_sets, din, list_K, n_runs, batch_size,
                                                mode, sets_per_call, select_of_K,
                                                step0=wi * len(list_K))
    return _two_dicts(rand, det, list_K, json_files)


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
    n_sets, npts_all, din, default_n = _set_geometry(x, tarr is not None)
    list_K = _norm_list_K(list_K, default_n, npts_all)
    full = (n_sets // batch_size) * batch_size
    data = {}
    if full == 0:
        data = {K: [float("nan"), 0] for K in list_K}
    else:
        # pass 1: the key of every set, resident
        key = torch.empty((full, npts_all), dtype=torch.float32, device=dev)
        cap = _sets_per_call(model, npts_all, mode, sets_per_call)
        engines = _engine_cache(model, npts_all, mode, dev, ((npts_all, din), torch.float32))
        for p0 in range(0, full, cap):
            b = min(cap, full - p0)
            eng, X = engines(b)
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


def most_peaks(F: int, Nt: int = 1) -> int:
    """The most peaks a set of Nt frames of F bins can hold: ceil((F - 2) / 2) per frame (two neighbouring
    bins are never both peaks, and the edge bins never are)."""
    return (int(F) - 1) // 2 * int(Nt)


@torch.no_grad()
def peak_sweep(model, spec, labels, farr, tarr=None, list_K: Optional[Iterable[int]] = None,
               radius_f: int = 1, radius_t: int = 0, rel_floor: float = float("inf"),
               abs_floor: float = float("-inf"), refine: bool = True, batch_size: int = 8,
               mode: int = _lib.MODE_F32, json_file: Optional[str] = None,
               sets_per_call: Optional[int] = None):
    """Accuracy of ``model`` on point sets reduced to their K strongest spectral peaks
    (``pca_hip.peak_points``: local maxima of the log-magnitude within ``radius_f`` bins and ``radius_t``
    frames, above the floors, frequency and level refined by a parabola when ``refine``), for every K in
    ``list_K``.  **No reference counterpart**: a fourth curve beside random-K, max-K and attention-K, and
    the first whose points leave the STFT grid.

    Arguments as subsample_sweep: FST ``spec`` [F, T] frames with ``tarr`` None, 3ST ``spec`` [F, Nt, S]
    chunks with ``tarr`` [Nt]; F >= 3.  Default list_K: default_list_K(most_peaks(F, Nt)), the most peaks a
    set can hold.

    For every K the sets are packed piece by piece, reduced by ``peak_points`` at that K, evaluated by
    ``STEngine.forward(X, lengths)`` at N = K - a set with fewer than K peaks is padded and its count masks
    the padding; a set without any peak is its one largest point - and tallied by pca_eval_tally.  One host
    read per K: the tally and the sum of the point counts together.

    Returns (and, with ``json_file``, writes) the max-K shape with the sets' mean size beside it:
    ``{"data": {K: [acc, 0]}, "list_K": [...], "mean_points": {K: mean points per scored set}}``."""
    dev = _model_device(model)
    x, lab, f32, t32 = _resident_sets(spec, labels, farr, tarr, dev)
    n_sets, npts_all, din, _ = _set_geometry(x, tarr is not None)
    F, Nt = int(x.shape[0]), (int(x.shape[1]) if tarr is not None else 1)
    list_K = _norm_list_K(list_K, most_peaks(F, Nt), npts_all)
    pca_hip.ops.peak_spec(radius_f, radius_t, rel_floor, abs_floor, refine)          # ValueError
    full = (n_sets // batch_size) * batch_size
    data, mean_points = {}, {}
    full_buf = {}

    def select_of_K(K, acc):
        def select(slot, draw, pos, out, labels_out, lengths_out):
            n = pos.numel()
            if n not in full_buf:              # the full-size sets of a piece
                full_buf[n] = torch.empty((n, npts_all, din), dtype=torch.float32, device=dev)
            _pack_sets(x, f32, t32, pos, full_buf[n])
            pca_hip.peak_points(full_buf[n], F, Nt, K, radius_f, radius_t, rel_floor, abs_floor, refine,
                                out=out, lengths_out=lengths_out)
            torch.index_select(lab, 0, pos, out=labels_out)
            acc[1:] += lengths_out.sum()
        return select

    for K in list_K:
        if full == 0:
            data[K], mean_points[K] = [float("nan"), 0], float("nan")
            continue
        acc = torch.zeros(2, dtype=torch.int64, device=dev)         # [correct, points]
        _run_pieces(model, K, din, mode, _sets_per_call(model, K, mode, sets_per_call),
                    [(0, 0, 0, full)], select_of_K(K, acc), acc, with_lengths=True)
        correct, points = acc.tolist()                              # the one host read of this K
        data[K], mean_points[K] = [correct / full, 0], points / full
    out = {"data": data, "list_K": list_K, "mean_points": mean_points}
    _write_json(out, json_file)
    return out


@torch.no_grad()
def reassign_sweep(model, clips: Sequence[torch.Tensor], labels: Sequence[int], fs: float, n_fft: int,
                   Ntemp: Optional[int] = None, list_strength: Iterable[float] = (0, .25, .5, .75, 1),
                   batch_size: int = 8, json_file: Optional[str] = None, mode: int = _lib.MODE_F32,
                   sets_per_call: Optional[int] = None, hop: Optional[int] = None,
                   drop_nyquist: bool = False, norm: str = "n_fft", **spec) -> Dict:
    """Accuracy of ``model`` as its inputs slide from the STFT grid (strength 0: the grid rows, bit for bit)
    to full time-frequency reassignment (strength 1; ``pca_hip.frame_points_reassigned``).  **No reference
    counterpart**: the reference's sets are grid points.

    ``clips`` / ``labels`` / ``fs`` / ``n_fft`` [/ ``hop`` / ``norm``] as ``ESC_wave_pc`` takes them; with
    ``Ntemp`` the 3-D sets of ``ESC_wave_pc_temp`` (Nyquist dropped), else the 2-D sets
    (``drop_nyquist``).  ``spec``: the other fields of ``reassign`` (axes, rel_floor, abs_floor, max_df,
    max_dt; the datasets' defaults).  The corpus is resident once; every strength is one
    ``_dataset_accuracy`` pass over a ``with_reassign`` view of it, one host read each.

    Returns (and, with ``json_file``, writes)
    ``{"data": {strength: [acc, 0]}, "list_strength": [...], "spec": {...}}``."""
    if "strength" in spec:
        raise ValueError("strength is the swept axis: pass list_strength")
    dev = _model_device(model)
    if Ntemp is None:
        ds = ESC_wave_pc(clips, labels, fs, n_fft, hop=hop, drop_nyquist=drop_nyquist, norm=norm,
                         device=dev, reassign=dict(spec))
    else:
        ds = ESC_wave_pc_temp(clips, labels, fs, n_fft, Ntemp, hop=hop, norm=norm, device=dev,
                              reassign=dict(spec))
    din = 2 if Ntemp is None else 3
    list_strength = [float(v) for v in list_strength]
    data = {}
    for strength in list_strength:
        view = ds.with_reassign(dict(spec, strength=strength))                      # ValueError
        data[strength] = [_dataset_accuracy(model, view, None, din, batch_size, mode, sets_per_call), 0]
    shown = {k: (v if isinstance(v, str) or math.isfinite(v) else str(v))
             for k, v in ds.reassign.items() if k != "strength"}
    out = {"data": data, "list_strength": list_strength, "spec": shown}
    _write_json(out, json_file)
    return out


def default_level_subsets(n_levels: int) -> List[tuple]:
    """Every single level, then every set with one level left out (without repeats, without the full set)."""
    singles = [(k,) for k in range(n_levels)]
    rest = [tuple(q for q in range(n_levels) if q != k) for k in range(n_levels)]
    return singles + [s for s in rest if s and s not in singles and len(s) < n_levels]


@torch.no_grad()
def multires_sweep(model, clips: Sequence[torch.Tensor], labels: Sequence[int], fs: float, levels, span: int,
                   subsets: Optional[Iterable[Iterable[int]]] = None, batch_size: int = 8,
                   json_file: Optional[str] = None, mode: int = _lib.MODE_F32,
                   sets_per_call: Optional[int] = None, **dataset_kw) -> Dict:
    """Accuracy of ``model`` over multi-resolution point sets (``ESC_wave_pc_multires``) when it sees all
    levels and when it sees each of ``subsets`` of them (default: ``default_level_subsets``): which
    resolutions a model trained on the mixed set leans on.  **No reference counterpart**: Code/pceval.py:55-105
    varies the analysis length one at a time.

    ``clips`` / ``labels`` / ``fs`` / ``levels`` / ``span`` and ``dataset_kw`` (norm, time_axis, ...) as the
    dataset takes them.  The corpus is resident once; every entry is one ``_dataset_accuracy`` pass over a
    ``with_levels`` view of it, one host read each.

    Returns (and, with ``json_file``, writes) ``{"data": {"0+1": [acc, 0], "0": [acc, 0], ...},
    "list_subsets": [[0, 1], [0], ...], "levels": [...], "span": span}``: the key joins a subset's level
    positions with "+", the full set first."""
    ds = ESC_wave_pc_multires(clips, labels, fs, levels, span, device=_model_device(model),
                              **dataset_kw)
    n = len(ds.layout["n_fft"])
    full = tuple(range(n))
    subsets = default_level_subsets(n) if subsets is None else [tuple(int(k) for k in s) for s in subsets]
    list_subsets = [full] + [s for s in subsets if s != full]
    din = 3 if ds.time_axis else 2
    data = {}
    for s in list_subsets:
        view = ds if s == full else ds.with_levels(s)                               # ValueError
        data["+".join(str(k) for k in s)] = [
            _dataset_accuracy(model, view, None, din, batch_size, mode, sets_per_call), 0]
    shown = [dict(n_fft=ds.layout["n_fft"][r], hop=ds.layout["hop"][r], Ntemp=ds.layout["Ntemp"][r],
                  F=ds.layout["F"][r], offset=ds.layout["offset"][r],
                  win_lengths=list(ds.layout["win_lengths"][r])) for r in range(n)]
    out = {"data": data, "list_subsets": [list(s) for s in list_subsets], "levels": shown, "span": int(span)}
    _write_json(out, json_file)
    return out


@torch.no_grad()
def band_sweep(model, clips: Sequence[torch.Tensor], labels: Sequence[int], fs: float, n_fft: int, banks,
               Ntemp: Optional[int] = None, batch_size: int = 8, json_file: Optional[str] = None,
               mode: int = _lib.MODE_F32, sets_per_call: Optional[int] = None, hop: Optional[int] = None,
               norm: str = "n_fft", **mel_kw) -> Dict:
    """Accuracy of ``model`` on band point sets (``pca_hip.frame_points_bands``: log-mel and other filter
    banks) for every bank of ``banks``: the band count as one more resolution axis - a Set Transformer
    trained at 64 bands can be scored at 32 or 128, since it takes any N.  **No reference counterpart**: the
    reference's sets have one point per FFT bin.

    ``clips`` / ``labels`` / ``fs`` / ``n_fft`` [/ ``hop`` / ``norm``] as ``ESC_wave_pc`` takes them; with
    ``Ntemp`` the 3-D sets of ``ESC_wave_pc_temp``, else the 2-D sets.  ``banks``: a dict name ->
    ``pca_hip.FilterBank``, or a list of ``n_mels`` - then every bank is ``pca_hip.mel_bank(fs, n_fft,
    n_mels, **mel_kw)`` (fmin, fmax, htk, norm as ``mel_norm``, power, amin) under the name ``str(n_mels)``.
    The corpus is resident once; every bank is one ``_dataset_accuracy`` pass over a ``with_bands`` view of
    it, one host read each.

    Returns (and, with ``json_file``, writes) ``{"data": {name: [acc, 0]}, "list_banks": [names],
    "banks": [{"n_bands", "power", "amin", "nnz"}, ...]}``, the banks in the order given."""
    if isinstance(banks, dict):
        if mel_kw:
            raise ValueError(f"band_sweep: {sorted(mel_kw)} describe mel banks; banks is a dict of FilterBanks")
        named = [(str(k), b) for k, b in banks.items()]
    else:
        if "mel_norm" in mel_kw:
            mel_kw["norm"] = mel_kw.pop("mel_norm")
        named = [(str(int(n)), pca_hip.mel_bank(fs, n_fft, int(n), **mel_kw)) for n in banks]   # ValueError
    if not named:
        raise ValueError("band_sweep: no banks")
    dev = _model_device(model)
    if Ntemp is None:
        ds = ESC_wave_pc(clips, labels, fs, n_fft, hop=hop, norm=norm, device=dev)
    else:
        ds = ESC_wave_pc_temp(clips, labels, fs, n_fft, Ntemp, hop=hop, norm=norm, device=dev)
    din = 2 if Ntemp is None else 3
    data = {}
    for name, bank in named:
        view = ds.with_bands(bank)                                                  # ValueError
        data[name] = [_dataset_accuracy(model, view, None, din, batch_size, mode, sets_per_call), 0]
    out = {"data": data, "list_banks": [name for name, _ in named],
           "banks": [bank.summary() for _, bank in named]}
    _write_json(out, json_file)
    return out


@torch.no_grad()
def pcen_sweep(model, clips: Sequence[torch.Tensor], labels: Sequence[int], fs: float, n_fft: int, bank, specs,
               Ntemp: Optional[int] = None, batch_size: int = 8, json_file: Optional[str] = None,
               mode: int = _lib.MODE_F32, sets_per_call: Optional[int] = None, hop: Optional[int] = None,
               norm: str = "n_fft") -> Dict:
    """Accuracy of ``model`` on band point sets of one ``bank`` whose value column is the log of the band
    energy (the first column, ``"log"``) and then per-channel energy normalisation for every ``pca_hip.Pcen``
    of ``specs`` (``pca_hip.frame_points_pcen``).  **No reference counterpart**.

    ``clips`` / ``labels`` / ``fs`` / ``n_fft`` [/ ``hop`` / ``norm``] / ``Ntemp`` as ``band_sweep`` takes
    them; ``specs``: a dict name -> ``Pcen``, or a list of ``Pcen`` (named ``"pcen0"``, ``"pcen1"``, ...); a
    ``None`` among them is the log-band dataset again.  The corpus is resident once; every column is one
    ``_dataset_accuracy`` pass over a ``with_pcen`` view of it, one host read each.

    Returns (and, with ``json_file``, writes) ``{"data": {name: [acc, 0]}, "list_specs": [names],
    "specs": [None or the spec's fields, ...], "bank": {...}}``, ``"log"`` first, then the specs in the
    order given."""
    named = list(specs.items()) if isinstance(specs, dict) else [(f"pcen{i}", p) for i, p in enumerate(specs)]
    named = [("log", None)] + [(str(k), p) for k, p in named]
    if len(named) < 2:
        raise ValueError("pcen_sweep: no specs")
    if len({k for k, _ in named}) != len(named):
        raise ValueError("pcen_sweep: two columns of one name ('log' is the log-band column)")
    for k, p in named:
        if p is not None and not isinstance(p, pca_hip.Pcen):
            raise TypeError(f"pcen_sweep: spec {k!r} is a {type(p).__name__}, expected a pca_hip.Pcen or None")
    dev = _model_device(model)
    if Ntemp is None:
        ds = ESC_wave_pc(clips, labels, fs, n_fft, hop=hop, norm=norm, device=dev, bands=bank)   # ValueError
    else:
        ds = ESC_wave_pc_temp(clips, labels, fs, n_fft, Ntemp, hop=hop, norm=norm, device=dev, bands=bank)
    din = 2 if Ntemp is None else 3
    data = {}
    for name, spec in named:
        data[name] = [_dataset_accuracy(model, ds.with_pcen(spec), None, din, batch_size, mode, sets_per_call), 0]
    out = {"data": data, "list_specs": [name for name, _ in named],
           "specs": [None if p is None else p.summary() for _, p in named], "bank": bank.summary()}
    _write_json(out, json_file)
    return out


@torch.no_grad()
def delta_sweep(model, clips: Sequence[torch.Tensor], labels: Sequence[int], fs: float, n_fft: int, widths,
                axes: str = "t", bank=None, Ntemp: Optional[int] = None, batch_size: int = 8,
                json_file: Optional[str] = None, mode: int = _lib.MODE_F32,
                sets_per_call: Optional[int] = None, hop: Optional[int] = None, norm: str = "n_fft",
                drop_nyquist: bool = False) -> Dict:
    """Accuracy of ``model`` on point sets with delta columns (``pca_hip.frame_points_delta``) for every
    regression width of ``widths`` (each in 1..4) at fixed ``axes``, so every column has the model's ``din``:
    2 (``Ntemp`` None) or 3, plus ``len(axes)``.  **No reference counterpart**.

    ``clips`` / ``labels`` / ``fs`` / ``n_fft`` [/ ``hop`` / ``norm``] / ``Ntemp`` as ``band_sweep`` takes
    them; ``bank``: a ``pca_hip.FilterBank`` for band sets, None for grid sets (``drop_nyquist`` as
    ``ESC_wave_pc`` takes it).  The corpus is resident once; every width is one ``_dataset_accuracy`` pass over
    a ``with_deltas`` view of it, one host read each.

    Returns (and, with ``json_file``, writes) ``{"data": {name: [acc, 0]}, "list_specs": [names],
    "specs": [the spec's fields, ...], "bank": {...} or None}``, the widths in the order given, named
    ``"w1"``, ``"w2"``, ..."""
    named = [(f"w{int(w)}", pca_hip.Deltas(axes, w)) for w in widths]                     # ValueError
    if not named:
        raise ValueError("delta_sweep: no widths")
    if len({k for k, _ in named}) != len(named):
        raise ValueError("delta_sweep: a width given twice")
    dev = _model_device(model)
    if Ntemp is None:
        ds = ESC_wave_pc(clips, labels, fs, n_fft, hop=hop, drop_nyquist=drop_nyquist, norm=norm, device=dev,
                         bands=bank, deltas=named[0][1])                                  # ValueError
    else:
        ds = ESC_wave_pc_temp(clips, labels, fs, n_fft, Ntemp, hop=hop, norm=norm, device=dev, bands=bank,
                              deltas=named[0][1])
    data = {}
    for name, spec in named:
        data[name] = [_dataset_accuracy(model, ds.with_deltas(spec), None, ds.din, batch_size, mode,
                                        sets_per_call), 0]
    out = {"data": data, "list_specs": [name for name, _ in named],
           "specs": [p.summary() for _, p in named], "bank": None if bank is None else bank.summary()}
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


def _chunk_labels(clips, labels, hop: int, Ntemp: int, foff, dev):
    """(S, labels int64 [S], ids of the whole chunks in corpus order; both on ``dev``) of the S
    Ntemp-frame chunk slots of a frame-aligned STFT (stft_logmag_batch(..., frame_align=Ntemp), frame
    offsets ``foff`` = chunk_plan's): a whole chunk carries its clip's label, every other slot -1."""
    frames = [int(pca_hip.lib().pca_stft_num_frames(int(x.numel()), hop)) for x in clips]
    plan_off, ids, clip_of = chunk_plan(frames, Ntemp)
    assert plan_off == foff, (plan_off, foff)
    S = foff[-1] // Ntemp
    lab = np.full(S, -1, dtype=np.int64)
    lab[ids] = np.asarray([int(labels[c]) for c in clip_of], dtype=np.int64)
    return S, torch.as_tensor(lab).to(dev), torch.as_tensor(np.asarray(ids, dtype=np.int64)).to(dev)


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
    S, lab, ids = _chunk_labels(clips, labels, hop, Ntemp, foff, spec.device)
    F = n_fft // 2
    farr, tarr = temporal_axes(fs, N, Ntemp, hf, F)
    return ESC_pc_temp.from_device(spec.view(S, Ntemp, F), lab, farr, tarr), ids


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
    def acc_of_N(at_rate, F, N):
        ds, ids = temporal_dataset(at_rate, labels, F, N, Ntemp, hf)
        # pc_temp3d_eval.py:93-94: no short batch
        return _dataset_accuracy(model, ds, ids, 3, batch_size, mode, sets_per_call)

    return _reframe_driver(clips, labels, fs, list_N, list_Fs, trim_dB, None, json_file, acc_of_N)


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
    logits, engines, done = None, _engine_cache(model, npts, mode, dev), 0
    while done < n_sets:
        b = min(cap, n_sets - done)
        eng = engines(b)[0]
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
    x, lab = _set_contiguous(spec, labels, eng.dev, eng.cnn)
    n_sets, n_cells, _, default_n = _set_geometry(x, eng.cnn)
    list_K = _norm_list_K(list_K, default_n, n_cells)

    def run_K(K, pieces, counts):
        _baseline_run(eng, x, lab, None, pieces, counts, K,
                      lambda slot: pca_hip.MAXK if slot == n_runs else pca_hip.RANDK, seed,
                      sets_per_call)

    rand, det = _k_passes(_baseline_full(eng, n_sets), list_K, n_runs, eng.dev, run_K)
    return _two_dicts(rand, det, list_K, json_files)


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
    S, lab, ids = _chunk_labels(clips, labels, hop, Ntemp, foff, spec.device)
    return spec.view(S, Ntemp, n_fft // 2).permute(2, 1, 0), lab, ids


@torch.no_grad()
def _baseline_reframe(eng: BaselineEngine, clips, labels, fs, list_N, hf, list_Fs, json_file,
                      n_fft, sets_per_call, trim_dB):
    """Experiment 1 of both baselines on _reframe_driver: an N is one _baseline_run pass over
    baseline_frames (FB) or baseline_chunks (CNN_temp) and one host read."""
    if n_fft is None:
        n_fft = 2 * eng.Nf if eng.cnn else 2 * (eng.layer_dims[0] - 1)

    def acc_of_N(at_rate, F, N):
        if eng.cnn:
            x, lab, ids = baseline_chunks(at_rate, labels, N, n_fft, eng.Nt, hf)
            n_sets = ids.numel()
        else:
            x, lab = baseline_frames(at_rate, labels, N, n_fft, hf)
            ids, n_sets = None, x.shape[1]
        full = _baseline_full(eng, n_sets)
        if full == 0:
            return float("nan")
        counts = torch.zeros(1, dtype=torch.int64, device=eng.dev)
        _baseline_run(eng, x, lab, ids, [(0, 0, 0, full)], counts, cap=sets_per_call)
        return int(counts.item()) / full                      # the one host sync of this N

    # Code/baseline_eval.py:74: trim, then resample; the trim is checked against the model's window
    return _reframe_driver(clips, labels, fs, list_N, list_Fs, trim_dB, n_fft, json_file, acc_of_N)


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
    return _baseline_reframe(eng, clips, labels, fs, list_N, hf, list_Fs, json_file, n_fft,
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
    return _baseline_reframe(eng, clips, labels, fs, list_N, hf, list_Fs, json_file, n_fft,
                             sets_per_call, trim_dB)
