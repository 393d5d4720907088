"""``train()`` with the reference's keyword API (run.py:30-400) on the HIP engine.

Differences from the reference are limited to what the hot-path scope excludes: no plots
(matplotlib figures) other than the loss landscape's.  ``visualization=True`` (run.py:192-208) evaluates
the loss-landscape plane after the fit on the device (engine.SirenEngine.loss_plane; the directions are
landscape.plane_directions, restated from the published filter-normalised definition because
loss_landscapes is not a dependency) and writes landscape.npy and, with matplotlib, landscape.png.
loss_mode 'mse' and 'mae' (L1Loss, run.py:161-163) at
alpha=0 are fused on device (at alpha=0 the reference's STFT term contributes exactly zero, SURVEY
§8 a8).  The reference's other loss options -- ``alpha > 0`` (auraloss.freq.STFTLoss, run.py:128,
:160) and ``loss_mode='snr'`` (auraloss.time.SNRLoss, run.py:126, :165) -- are refused unless
``restated_losses=True``: auraloss is not a dependency of this project, so those two terms are
restated from their published 0.4.0 definitions (csrc/stft.hip) and parity is to that formula, not to
an installed module; the switch makes that substitution explicit.  ``num_freq=F``
puts the Gaussian random-Fourier-feature encoding of run.py:141-144 in front of the waveform MLP
(encoding.GaussianEncoding; its b is saved in the checkpoint, which the reference forgets).
``multichannel=True`` (keyword-only) fits the (time,
channel) grid of MultiWaveformFitting (utils.py:186-231; the reference's call site,
run.py:59-63, is commented out, with mode == 'lp' selecting its FIR decimation) -- BASELINE
cfg3's data path; its output.wav is written as a (samples, channels) file.  arch='kan' fits KAN([1, H, H, 1]) (SURVEY §8 f4,
kan.py) on its own fp32 HIP kernels.  method='mdct' fits the
MDCT-domain target (utils.MDCTFitting, N = 2048, mode='log' = takelog) with
(bin, frame) coordinates and inverts it as run.py:258-290 does.  Everything the path
produces -- output.wav, the checkpoint dict, parameters.json with the run.py-formula SNR --
keeps the reference's names and formats.  One deliberate deviation: for method='mdct' the
reference's final SNR line (run.py:335) raises a numpy broadcast error whenever
fs * duration is not a multiple of N/2 (the recovered signal has frames * N/2 samples);
here the SNR is taken over the common length instead.
"""
from __future__ import annotations

import json
import os
import time

import numpy as np
import scipy.io.wavfile as wavfile
import torch

from .encoding import GaussianEncoding
from .engine import KanEngine, SirenEngine
from .kan import KAN, _hip_check_grid
from .models import SirenWithSnakeTanh
from .utils import (MDCTFitting, MultiWaveformFitting, WaveformFitting, calculate_snr, get_coord,
                    load_mono_like_librosa, reported_snr)


RFF_KEY = "rff_b"  # checkpoint key of the GaussianEncoding's b (an addition: run.py:359-362 saves none)


def save_parameters(experiment_folder, **kwargs):
    """run.py:25-28."""
    with open(f"{experiment_folder}/parameters.json", "w") as file:
        json.dump(kwargs, file, indent=4)


def _rank0() -> bool:
    d = torch.distributed
    return not (d.is_available() and d.is_initialized()) or d.get_rank() == 0


def _distributed() -> bool:
    d = torch.distributed
    return d.is_available() and d.is_initialized() and d.get_world_size() > 1


def _experiment_folder(experiment_path, inst, method, tag):
    """run.py:34-40 -- append '(2)' to the tag until the folder is new.  Under data
    parallelism rank 0 decides and broadcasts the tag, so every rank returns the same path."""
    if _rank0():
        folder = f"{experiment_path}/{inst}-{method}-{tag}"
        while os.path.exists(folder):
            tag = tag + "(2)"
            folder = f"{experiment_path}/{inst}-{method}-{tag}"
        os.makedirs(folder)
    if _distributed():
        box = [tag]
        torch.distributed.broadcast_object_list(box, src=0)
        tag = box[0]
    return tag, f"{experiment_path}/{inst}-{method}-{tag}"


def train(experiment_path: str, tag: str, inst: str, duration: int, num_channels=1, method='wave',
          arch='mlp', loss_mode='mse', mode=None, decimation=1, bwe=False, num_hidden_features=256,
          num_sine=2, num_snake=2, num_tanh=0, num_freq=None, omega=22000, first_linear=False,
          last_linear=True, hidden_omega=30, a_initial=0.5, total_steps=20000, learning_rate=1e-3,
          min_learning_rate=1e-6, alpha=0.0, prev_ckpt_path=None, visualization=False, *,
          filename=None, data_dir="data", seed=None, micro_batch=1 << 20, use_graph=True,
          device=None, verbose=False, multichannel=False, patience=200, restated_losses=False,
          stft_loss="stft", split_spectral=False, kan_grid_size=5, kan_prev_grid_size=None,
          kan_regrid_margin=0.01, keep_best=False):
    """Fit one clip; returns the checkpoint path (run.py:400).  Extra keyword-only knobs:
    ``filename`` (default ``{data_dir}/{inst}.wav`` as run.py:33), ``seed`` (torch.manual_seed
    before model construction), ``micro_batch`` (rows per fused micro-batch), ``use_graph``
    (replay each step as a HIP graph), ``device``, ``multichannel`` (the (t, ch) grid of
    MultiWaveformFitting, run.py:59-63), ``patience`` (ReduceLROnPlateau, run.py:117's 200),
    ``restated_losses`` (opt-in: fit with ``alpha > 0`` and / or ``loss_mode='snr'`` using this
    project's restatement of auraloss's STFTLoss / SNRLoss defaults -- run.py:126-128, :160-169 --
    instead of raising; parity is to the published formula, not to an installed auraloss.  For
    method 'wave' and 'mdct' of the MLP, the whole signal in one micro-batch on one GPU, and for
    arch='kan' together with ``split_spectral``; with 'snr'
    the loss is negative, so the dB history is NaN as in the reference, run.py:180),
    ``stft_loss`` (with ``restated_losses``: 'stft', the single STFTLoss() of run.py:128, or 'mrstft',
    the MultiResolutionSTFTLoss() of run.py:127 -- more than 1024 samples; recorded in parameters.json
    only when it is not 'stft'), ``split_spectral`` (with ``restated_losses``: the engines' split step,
    which fits with these losses across micro-batches and data-parallel ranks -- a clip longer than
    ``micro_batch``, or more than one GPU, and the only way arch='kan' fits with them; recorded in
    parameters.json only when true), ``kan_grid_size`` (arch='kan': the ``grid_size`` of KAN(...), 1 to 64;
    run.py:93 leaves it at kan.py's default 5; recorded in parameters.json only when it is not 5;
    ``prev_ckpt_path`` resumes a checkpoint of the same grid size), ``kan_prev_grid_size`` (arch='kan' with
    ``prev_ckpt_path``: the grid size the checkpoint was fitted at, for a coarse-to-fine grid curriculum such
    as 5 -> 10 -> 20: the KAN is built at that size, loaded, and refitted onto ``kan_grid_size`` over the run's
    coordinates by ``KAN.regrid``; Adam starts afresh, the checkpoint's moments having the old shapes; one
    process; both sizes are recorded in parameters.json when it is given.  None: the checkpoint is loaded
    into a model of ``kan_grid_size`` as before), ``kan_regrid_margin`` (that refit's ``margin``, kan.py:169's
    0.01 by default: an absolute pad of the knot range, which leaves a hidden input whose activations span
    less than about ``kan_grid_size`` x margin with an empty last knot span, and the refit then refuses it as
    rank deficient -- pass a smaller one, 0 included, for such a model; recorded when it is not 0.01),
    ``keep_best`` (run.py:171-174 as the reference meant it: its ``best_model = model`` is an alias, so the
    reference and, by default, this port write the LAST step's weights.  True keeps the weights of the
    step with the smallest loss of this run on the device, the first such step, decided and copied inside
    the step itself with no host read-back (engine keep_best), and restores them after the fit
    and its top-up: the landscape plane, output.wav, both SNRs and the checkpoint's model_state_dict are
    then the best step's; optimizer_state_dict stays the final Adam state as run.py:359-362 saves it.  Every
    arch, loss and data path the call otherwise takes; a resumed run starts from +inf, "best of this run".
    A fit that took no snapshot -- no step, or every loss NaN -- keeps its final weights.  parameters.json
    gains keep_best and best_loss only when it is set)."""
    if not isinstance(keep_best, bool):
        raise TypeError(f"keep_best={keep_best!r} must be a bool")
    if method not in ("wave", "mdct"):
        raise ValueError("specify the correct fitting method as wave or mdct (run.py:77-78)")
    if method == "mdct" and bwe:
        raise NotImplementedError("bwe is a waveform-mode feature (run.py:127-131)")
    if arch not in ("mlp", "kan"):
        raise NotImplementedError(f"arch={arch!r}: the reference builds 'kan' or the MLP (run.py:92-96)")
    if arch != "kan" and kan_grid_size != 5:
        raise ValueError(f"kan_grid_size={kan_grid_size!r} is the KAN's grid size: it needs arch='kan'")
    if kan_prev_grid_size is not None and (arch != "kan" or prev_ckpt_path is None):
        raise ValueError(f"kan_prev_grid_size={kan_prev_grid_size!r} is the grid size of the KAN checkpoint to refit: "
                         "it needs arch='kan' and prev_ckpt_path")
    if arch == "kan" and method == "mdct":
        raise NotImplementedError("arch='kan' takes 1-D coordinates (run.py:92 builds KAN([1, H, H, 1]))")
    spectral = loss_mode == "snr" or alpha != 0.0
    if loss_mode not in ("mse", "mae", "snr") or (spectral and not restated_losses):
        raise NotImplementedError("HIP path implements loss_mode 'mse' / 'mae' with alpha=0 (run.py:161-169); "
                                  "restated_losses=True fits 'snr' and alpha > 0 with the restated auraloss terms")
    if stft_loss not in ("stft", "mrstft"):
        raise ValueError(f"stft_loss={stft_loss!r}: 'stft' (run.py:128) or 'mrstft' (run.py:127)")
    if spectral and multichannel:
        raise NotImplementedError("restated_losses fits the waveform / MDCT MLP and the KAN (no multichannel)")
    if spectral and arch == "kan" and not split_spectral:
        raise NotImplementedError("arch='kan' is fitted with 'snr' and alpha > 0 by the phased step alone: add "
                                  "split_spectral=True to restated_losses=True")
    if multichannel and (method != "wave" or arch != "mlp" or bwe):
        raise NotImplementedError("multichannel fits the waveform MLP (run.py:59-63) without bwe")
    if num_freq is not None and (method != "wave" or arch != "mlp" or multichannel):
        # the reference's own code cannot run these: b is [num_freq][1] against 2-D coordinates
        # (run.py:142-143), and KAN is built with input width 1 (run.py:93)
        raise NotImplementedError("num_freq encodes the 1-D waveform coordinate of the MLP (run.py:141-144)")
    if visualization and arch == "kan":
        raise NotImplementedError("visualization=True (the loss-landscape plane, run.py:192-208) runs on the MLP's "
                                  "kernels: arch='kan' has no plane")

    filename = filename or f"{data_dir}/{inst}.wav"
    rank0 = _rank0()
    tag, experiment_folder = _experiment_folder(experiment_path, inst, method, tag)
    decimation = int(decimation)

    takelog = False
    if method == "wave" and multichannel:  # run.py:59-63 (commented out in the reference)
        input_data = MultiWaveformFitting(filename, duration=duration, num_channels=num_channels, lp=mode == "lp")
        model_input, samples = input_data[0]
        ground_truth = torch.from_numpy(np.ascontiguousarray(samples, dtype=np.float32))
        input_dimension = 2
    elif method == "wave":
        input_data = WaveformFitting(filename, duration=duration, decimation=decimation)
        model_input, ground_truth = input_data[0]
        input_dimension = 1
    else:  # run.py:67-76
        N = 2048
        takelog = mode == "log"
        input_data = MDCTFitting(filename, duration=duration, N=N, takelog=takelog)
        model_input, pixels = input_data[0]
        ground_truth = torch.from_numpy(np.ascontiguousarray(pixels))
        input_dimension = 2

    if alpha != 0.0 and stft_loss == "mrstft" and ground_truth.numel() <= 1024:
        raise ValueError(f"stft_loss='mrstft' needs more than 1024 samples (reflect padding of its 2048-point "
                         f"frame is undefined for {ground_truth.numel()}; torch.stft refuses it too)")

    if num_freq is not None:  # run.py:81-82
        input_dimension = num_freq * 2

    if seed is not None:
        torch.manual_seed(seed)
    if arch == "kan":  # run.py:92-93
        if kan_prev_grid_size is not None:
            _hip_check_grid(kan_grid_size, 3)  # the size to refit onto; the model below is the checkpoint's
        model = KAN([1, num_hidden_features, num_hidden_features, 1],
                    grid_size=kan_grid_size if kan_prev_grid_size is None else kan_prev_grid_size)
        model.hip_check()  # a grid size or order the HIP path refuses, before any data is read further
    else:
        model = SirenWithSnakeTanh(in_features=input_dimension, out_features=1,
                                   hidden_features=num_hidden_features, num_sine=num_sine,
                                   num_snake=num_snake, num_tanh=num_tanh, num_freq=num_freq,
                                   first_linear=first_linear, last_linear=last_linear,
                                   first_omega_0=omega, hidden_omega_0=hidden_omega, a_initial=a_initial)
    ckpt = None
    if prev_ckpt_path is not None:  # run.py:84-106
        ckpt = torch.load(prev_ckpt_path, map_location="cpu", weights_only=True)
        model.load_state_dict(ckpt["model_state_dict"])

    # run.py:141-144: the encoding is drawn after the model (sigma 10.0).  The reference forgets
    # to save its b, so a resumed run there fits against a fresh one; here the checkpoint carries
    # it under RFF_KEY and prev_ckpt_path reuses it (a checkpoint without the key draws afresh)
    encoding = None
    if num_freq is not None:
        saved_b = None if ckpt is None else ckpt.get(RFF_KEY)
        encoding = GaussianEncoding(b=saved_b) if saved_b is not None else GaussianEncoding(10.0, 1, num_freq)
        if encoding.encoded_size != num_freq:
            raise ValueError(f"checkpoint encoding has {encoding.encoded_size} frequencies, num_freq={num_freq}")

    dev = torch.device(device or "cuda")
    if kan_prev_grid_size is not None:
        # the checkpoint's curves refitted onto the new grid over the run's own coordinates; the
        # optimizer state has the old grid's shapes, so Adam starts afresh
        if torch.distributed.is_available() and torch.distributed.is_initialized():
            raise NotImplementedError("kan_prev_grid_size: the refit takes the order statistics of all coordinates "
                                      "in one process")
        model = model.to(dev).regrid(model_input.to(dev), kan_grid_size, margin=kan_regrid_margin)
        ckpt = None
    Engine = KanEngine if arch == "kan" else SirenEngine
    kw = {"loss_mode": loss_mode, "alpha": alpha}
    if arch != "kan":
        kw["encoding"] = encoding
    if stft_loss != "stft":
        kw["stft_loss"] = stft_loss
    if split_spectral:
        if not restated_losses:
            raise NotImplementedError("split_spectral is the restated_losses step across micro-batches and ranks")
        kw["split_spectral"] = True
    if keep_best:
        kw["keep_best"] = True
    engine = Engine(model, model_input, ground_truth, lr=learning_rate, min_lr=min_learning_rate,
                    patience=patience, micro_batch=micro_batch, hist_cap=total_steps, device=dev, **kw)
    if ckpt is not None:
        engine.load_adam_state_dict(ckpt["optimizer_state_dict"])

    torch.cuda.synchronize(dev)
    start_time = time.time()
    single = not (torch.distributed.is_available() and torch.distributed.is_initialized())
    if use_graph and single and total_steps > 1:
        engine.step()                    # step 0 eagerly (also warms up the kernels)
        engine.capture_graph()
        for _ in range(total_steps - 1):
            engine.step()
    else:
        for _ in range(total_steps):
            engine.step()
    # steps the fp16 range guard rejected were recomputed by the next call: top up to
    # total_steps applied optimizer steps (one host check, after the loop)
    while engine.steps_applied() < total_steps:
        engine.step()
    torch.cuda.synchronize(dev)
    end_time = time.time()
    total_time = (end_time - start_time) / 60

    # run.py:171-174: the reference hands best_model to the plane and to the inference below
    best_loss = None
    if keep_best:
        best_loss, best_step, _ = engine.best_info()
        if best_step >= 0:
            engine.load_best()
        else:
            best_loss = None

    # run.py:192-208: the loss-landscape plane around the fitted weights, after the timed fit.  The
    # directions are drawn on rank 0 (loss_plane broadcasts them) from the run's seed when it has one
    landscape_time = None
    if visualization:
        from .landscape import plane_directions, save_plane
        gen = None if seed is None else torch.Generator().manual_seed(seed)
        t0 = time.time()
        d1, d2 = plane_directions([p for _, p in model.named_parameters()], distance=2.0, steps=30, generator=gen)
        plane = engine.loss_plane(d1, d2, steps=30)   # synchronises: the plane comes back to the host
        landscape_time = time.time() - t0
        if rank0:
            save_plane(plane.numpy(), experiment_folder)

    raw_losses, raw_lrs = engine.history()
    with np.errstate(invalid="ignore"):  # 'snr': a negative loss gives NaN, as in the reference
        losses = 10 * np.log10(raw_losses.astype(np.float64) + 1e-10)   # run.py:180
    lrs = 10 * np.log10(raw_lrs)                                     # run.py:190
    best_iter = int(np.argmin(raw_losses)) if len(raw_losses) else -1
    if best_loss is not None:
        best_iter = best_step   # the same step: argmin and the device's strict < both pick the first minimum

    param_size = sum(p.nelement() * p.element_size() for p in model.parameters())
    buffer_size = sum(b.nelement() * b.element_size() for b in model.buffers())
    model_size = (param_size + buffer_size) / 1024

    # inference (run.py:251-256); best_model aliases the final model (run.py:173) unless keep_best
    # restored the best step's weights above
    if bwe:
        coords = get_coord(input_data.original_sample_rate * duration, dim=1)
        recover_sample_rate = input_data.original_sample_rate
    else:
        coords = model_input
        recover_sample_rate = input_data.sample_rate
    model_output = engine.infer(coords.to(dev)).cpu().numpy().astype(np.float32)
    if method == "wave" and multichannel:
        signal_recovered = input_data.to_channels(model_output)      # (samples, channels)
    elif method == "wave":
        signal_recovered = model_output
    else:  # run.py:258-259, 281-290 (double exp in log mode)
        signal_recovered = input_data.to_signal(model_output, takelog=takelog).reshape(-1)

    ckpt_path = f"{experiment_folder}/saved_ckpt.pt"
    if rank0:
        output_filename = f"{experiment_folder}/output.wav"
        wavfile.write(output_filename, recover_sample_rate,
                      signal_recovered if multichannel else signal_recovered.reshape(-1, 1))
        ref, fs_ref = load_mono_like_librosa(filename)
        rec, _ = load_mono_like_librosa(output_filename)
        if method == "mdct":
            m = min(int(fs_ref * duration), len(rec))
            ref, rec = ref[:m], rec[:m]
        # multichannel: librosa.load averages the channels of both files; mode 'lp' halved the rate
        d_snr = (2 if mode == "lp" else 1) if multichannel else decimation
        snr_final = float(reported_snr(ref, fs_ref, rec, duration, d_snr, bwe))
        target = ground_truth.numpy().reshape(-1)
        # the fit in its own (training) domain: waveform or normalised MDCT map
        snr_target = float(calculate_snr(target, model_output)) if not bwe else None

        checkpoint = {"model_state_dict": {k: v.detach().cpu().clone() for k, v in model.state_dict().items()},
                      "optimizer_state_dict": engine.adam_state_dict()}
        if encoding is not None:
            checkpoint[RFF_KEY] = encoding.b.detach().cpu().clone()
        torch.save(checkpoint, ckpt_path)

        n_gpus = torch.distributed.get_world_size() if not single else 1
        params = {
            "experiment_path": experiment_path, "tag": tag, "inst": inst, "duration": duration,
            "num_channels": num_channels, "method": method, "arch": arch, "loss_mode": loss_mode,
            "mode": mode, "decimation": decimation, "bwe": bwe,
            "num_hidden_features": num_hidden_features, "num_sine": num_sine,
            "num_snake": num_snake, "num_tanh": num_tanh, "num_freq": num_freq, "omega": omega,
            "hidden_omega": hidden_omega, "a_initial": a_initial, "total_steps": total_steps,
            "learning_rate": learning_rate, "min_learning_rate": min_learning_rate, "alpha": alpha,
            "prev_ckpt_path": prev_ckpt_path, "curr_ckpt_path": ckpt_path,
            "visualization": visualization, "parameter_size(KB)": param_size / 1024,
            "total_model_size(KB)": model_size, "total_trainig_time(min)": total_time,
            "SNR": snr_final,
            # additions of this build
            "SNR_target": snr_target, "best_iter": best_iter,
            "final_loss": float(raw_losses[-1]) if len(raw_losses) else None,
            "coord_samples_per_sec": engine.n_total * total_steps / max(total_time * 60, 1e-9),
            "n_gpus": n_gpus, "fp16_overflow_steps": engine.guard_state()["overflows"],
        }
        if stft_loss != "stft":
            params["stft_loss"] = stft_loss
        if kan_grid_size != 5 or kan_prev_grid_size is not None:
            params["kan_grid_size"] = kan_grid_size
        if kan_prev_grid_size is not None:
            params["kan_prev_grid_size"] = kan_prev_grid_size
            if kan_regrid_margin != 0.01:
                params["kan_regrid_margin"] = kan_regrid_margin
        if split_spectral:
            params["split_spectral"] = True
        if keep_best:
            params["keep_best"] = True
            params["best_loss"] = best_loss
        if visualization:
            params["landscape_time_s"] = landscape_time
        save_parameters(experiment_folder, **params)
        if verbose:
            print(json.dumps({"SNR": snr_final, "SNR_target": snr_target, "time_min": total_time}))
    train.last_history = (losses, lrs)
    return ckpt_path
