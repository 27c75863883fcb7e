"""Run files of a trained model: ``<ARCH>(<timestamp>)_net.pth`` + ``<ARCH>(<timestamp>)_config.json``
in the layout the reference's training scripts write and its evaluation scripts read.

Writer  <- ``Code/settransformer.py:134-162`` (FST) / ``Code/settransformertemp.py:147-177`` (3ST):
           ``torch.save(model.state_dict())`` of the DataParallel-wrapped model (keys carry the
           ``module.`` prefix) and a flat JSON dict of everything needed to rebuild it.
Reader  <- ``Code/pceval.py:23-47`` / ``Code/pc_temp3d_eval.py:23-49``: JSON -> ``ST(dim_hidden=dhidden,
           num_heads=nheads, num_inds=ninds)`` (3ST: ``dim_input=3``) -> ``nn.DataParallel`` ->
           ``load_state_dict``.

The key set and key order of the JSON follow the shipped files
(``Code/model_saves/FST(...)_config.json``: ``numpy_seed``; ``3ST(...)_config.json``: ``Ntemp`` after
``trim_dB`` and ``np_seed``), so either side of the pair can be swapped with the reference's.
Weights are read with ``torch.load(weights_only=True)`` only.

A run file holds what evaluation needs.  A *checkpoint* (``save_checkpoint`` / ``load_checkpoint``, no
reference counterpart) holds what the next training step needs - ``Trainer.state_dict()``: parameters,
Adam moments, step counters, the index stream's position, the running statistics - so that a run that
ends early continues bit for bit.
"""
import json
import os
from datetime import datetime
from typing import Dict, Optional, Tuple

import torch
from torch import nn

from models import ST

__all__ = ["ARCHITECTURES", "run_config", "save_run", "load_run", "save_checkpoint",
           "load_checkpoint"]

ARCHITECTURES = {
    "FST": "FST (Framewise Set Transformer)",
    "3ST": "3ST (Set Transformer Temporal)",
}


def run_config(arch: str, *, epochs: int, weight_decay: float, window_size: int,
               hop_factor: float, trim_dB: float, sampling_rate: int, classes: int, dhidden: int,
               nheads: int, ninds: int, batch_size: int, learning_rate: float, dataset: str,
               numpy_seed: int, torch_seed: int, model_params: int,
               Ntemp: Optional[int] = None) -> Dict:
    """The config dict of one run, keys in the order of the reference's writer."""
    if arch not in ARCHITECTURES:
        raise ValueError(f"unknown architecture {arch!r} (one of {sorted(ARCHITECTURES)})")
    if (arch == "3ST") != (Ntemp is not None):
        raise ValueError("Ntemp belongs to the 3ST config and only to it")
    c = dict(epochs=epochs, weight_decay=weight_decay, window_size=window_size,
             hop_factor=hop_factor, trim_dB=trim_dB)
    if arch == "3ST":
        c["Ntemp"] = Ntemp
    c.update(sampling_rate=sampling_rate, classes=classes, dhidden=dhidden, nheads=nheads,
             ninds=ninds, batch_size=batch_size, learning_rate=learning_rate, dataset=dataset,
             architecture=ARCHITECTURES[arch])
    # the temporal script names the numpy seed differently (settransformertemp.py:163)
    c["np_seed" if arch == "3ST" else "numpy_seed"] = numpy_seed
    c.update(torch_seed=torch_seed, model_params=model_params)
    return c


def _arch_of(config: Dict) -> str:
    for k, v in ARCHITECTURES.items():
        if config.get("architecture") == v:
            return k
    raise ValueError(f"not a Set Transformer run: architecture = {config.get('architecture')!r}")


def save_run(model, config: Dict, directory: str, now: Optional[datetime] = None,
             state_dict: Optional[Dict] = None) -> Tuple[str, str]:
    """Write the weight and config files of a run; returns (pth path, json path).

    ``model`` may be an ``ST`` or its ``nn.DataParallel`` wrapper; the file always holds the
    wrapped key names, like the reference's.  ``state_dict``: the weights to write instead of the
    model's own, under the model's keys (``Trainer.averaged_state_dict()``)."""
    arch = _arch_of(config)
    sd = model.state_dict() if state_dict is None else dict(state_dict)
    wrapped = isinstance(model, nn.DataParallel) if state_dict is None else \
        all(k.startswith("module.") for k in sd)
    if not wrapped:
        sd = {"module." + k: v for k, v in sd.items()}
    sd = {k: v.detach().to("cpu").contiguous() for k, v in sd.items()}
    stamp = str(now or datetime.now())
    os.makedirs(directory, exist_ok=True)
    stem = os.path.join(directory, f"{arch}({stamp})")
    torch.save(sd, stem + "_net.pth")
    with open(stem + "_config.json", "w") as fp:
        json.dump(config, fp)
    return stem + "_net.pth", stem + "_config.json"


def load_run(json_path: str, pth_path: Optional[str] = None, device=None,
             dim_output: Optional[int] = None):
    """(DataParallel-wrapped ST, config) of a run.  ``pth_path`` defaults to the JSON's sibling;
    ``device`` defaults to the current HIP device when there is one (the engine and
    ``evalsweep.reframe_sweep`` take the wrapped model as it is), else the CPU.

    The evaluation scripts build the model with the default ``dim_output=10``; ``dim_output``
    overrides it, otherwise it is read off the classifier weight in the file."""
    with open(json_path) as fp:
        config = json.load(fp)
    arch = _arch_of(config)
    if pth_path is None:
        pth_path = json_path[: -len("_config.json")] + "_net.pth"
    sd = torch.load(pth_path, map_location="cpu", weights_only=True)
    if not all(k.startswith("module.") for k in sd):
        sd = {"module." + k: v for k, v in sd.items()}
    if dim_output is None:
        dim_output = int(sd["module.dec.1.weight"].shape[0])
    if device is None:
        device = "cuda" if torch.cuda.is_available() else "cpu"
    model = ST(dim_input=3 if arch == "3ST" else 2, dim_output=dim_output,
               dim_hidden=config["dhidden"], num_heads=config["nheads"],
               num_inds=config["ninds"]).to(device)
    model = nn.DataParallel(model)
    model.load_state_dict(sd)
    return model, config


def save_checkpoint(path: str, trainer, config: Optional[Dict] = None) -> str:
    """Write ``trainer.state_dict()`` (and the run's config dict, if given) to ``path`` with
    ``torch.save``: tensors and plain values only.  Written to a sibling file first and renamed, so a
    run that is stopped while writing leaves the previous checkpoint whole.  Returns ``path``."""
    state = dict(trainer=trainer.state_dict(), config=config)
    directory = os.path.dirname(os.path.abspath(path))
    os.makedirs(directory, exist_ok=True)
    tmp = path + ".part"
    torch.save(state, tmp)
    os.replace(tmp, path)
    return path


def load_checkpoint(path: str, trainer) -> Optional[Dict]:
    """Put ``trainer`` where the checkpoint's run stopped (``Trainer.load_state_dict``: a mismatch of
    batch size, set size, mode or world size raises and names the field).  Read with
    ``torch.load(weights_only=True)``.  Returns the config stored with it, or None."""
    state = torch.load(path, map_location="cpu", weights_only=True)
    trainer.load_state_dict(state["trainer"])
    return state.get("config")
