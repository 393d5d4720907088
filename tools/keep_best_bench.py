"""What keep_best=True costs a graph-replayed step.

    python tools/keep_best_bench.py [--takes 5] [--reps 10] [--out FILE]

Per shape -- cfg2 (SIREN 5 x 1024, 2^20 coordinates), the width-256 live stack at 441 000, KAN([1, 64, 64, 1])
at 441 000 -- three engines from one seed in one process, each warm and replaying its captured step:

  off     keep_best=False: the step as it always was
  idle    keep_best=True, the best loss held at -inf: every block of the copy reads its three scalars
          and returns, the commit thread likewise (a step that does not improve)
  take    keep_best=True, the best loss put back to +inf in every step: every step copies
          n_params floats (a step that improves)

The one-word write that holds the best loss is captured at the head of each engine's update (the off engine
writes a scratch word instead, so all three replay the same extra node): nothing is launched between two
replays of a graph.

`takes` rounds visit the three in turn (off, idle, take, off, ...), each round the median of `reps` replays
by device events; the figures are the medians over the rounds, the off engine's own spread over its rounds
(max - min) beside the differences.  Then siren_best_keep alone on the same vectors, `reps` calls back to
back between two events: the pair's own time with and without the copy, i.e. what of the difference is copy
and what is launch.  The byte bound: a taking step reads and writes n_params floats, 8 n_params bytes, at the
8 TB/s HBM peak; an idle one reads three scalars.  One JSON line."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_PEAK = 8.0e12   # bytes / s (MI355X)
NEG_INF_BITS = -8388608   # 0xFF800000 as int32: no loss is below it


def data(rows):
    t = torch.linspace(-1, 1, rows).reshape(-1, 1)
    return t, (0.5 * torch.sin(2300.0 * t) + 0.3 * torch.sin(7100.0 * t + 0.5)).reshape(-1)


def make(shape, dev, keep_best):
    from inr_for_audio_amd.engine import KanEngine, SirenEngine
    from inr_for_audio_amd.kan import KAN
    from inr_for_audio_amd.models import SirenWithSnakeTanh
    torch.manual_seed(0)
    if shape == "cfg2":
        x, y = data(1 << 20)
        m = SirenWithSnakeTanh(1, 1, 1024, 4, 0, 0, first_omega_0=3000.0, hidden_omega_0=30.0)
        return SirenEngine(m, x, y, device=dev, keep_best=keep_best)
    if shape == "live":
        x, y = data(441_000)
        m = SirenWithSnakeTanh(1, 1, 256, 0, 4, 0, first_omega_0=22000.0, hidden_omega_0=30.0, a_initial=0.5)
        return SirenEngine(m, x, y, device=dev, keep_best=keep_best)
    x, y = data(441_000)
    return KanEngine(KAN([1, 64, 64, 1]), x, y, device=dev, keep_best=keep_best)


def hold(eng, mode):
    """Enqueue the best state a mode wants: (-inf: never taken) or (+inf: always taken)."""
    if mode == "idle":
        eng._best[:1].fill_(NEG_INF_BITS)
    elif mode == "take":
        eng._best[:1].copy_(eng._best_init[:1])
    else:
        eng._scratch_word.fill_(NEG_INF_BITS)


def hold_in_update(eng, mode):
    """The mode's one-word write at the head of the engine's update, so that capture_graph records it."""
    eng._scratch_word = torch.zeros(1, dtype=torch.int32, device=eng.device)
    update = eng._launch_update

    def launch_update():
        hold(eng, mode)
        update()
    eng._launch_update = launch_update


def replay_ms(eng, reps):
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        eng.step()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms)


def pair_alone_us(eng, mode, reps):
    """siren_best_keep by itself, `reps` calls between two events (idle: none copies; take: the first call
    copies and commits, so the state is put back between the calls)."""
    from inr_for_audio_amd._lib import check, ptr
    lay, s = eng.layout, torch.cuda.current_stream(eng.device).cuda_stream
    sse = eng.grads.data_ptr() + 4 * lay.sse_offset
    eng.grads[lay.sse_offset + 1] = 0.0   # a live guard's stall slot is not what is measured

    def call():
        check(eng.lib.siren_best_keep(ptr(eng.params), ptr(eng.best_params), lay.n_params, ptr(eng.state), sse, 1.0,
                                      None, ptr(eng._best), s), "siren_best_keep")
    hold(eng, mode)
    call()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        hold(eng, mode)
        call()
    b.record()
    torch.cuda.synchronize()
    with_hold = a.elapsed_time(b)
    a.record()
    for _ in range(reps):
        hold(eng, mode)
    b.record()
    torch.cuda.synchronize()
    return (with_hold - a.elapsed_time(b)) * 1e3 / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--takes", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--shapes", default="cfg2,live,kan64")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import __graft_entry__ as ge
    ge.build(diag=False)
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "takes": a.takes, "reps": a.reps, "shapes": {}}
    for shape in a.shapes.split(","):
        engs = {"off": make(shape, dev, False), "idle": make(shape, dev, True), "take": make(shape, dev, True)}
        for m, eng in engs.items():
            hold_in_update(eng, m)
            eng.step()
            eng.capture_graph()
            for _ in range(3):
                eng.step()
        rounds = {m: [] for m in engs}
        for _ in range(a.takes):
            for m, eng in engs.items():
                rounds[m].append(replay_ms(eng, a.reps))
        med = {m: statistics.median(v) for m, v in rounds.items()}
        n = engs["take"].layout.n_params
        # the modes did what they are named for: every timed step of `take` copied, none of `idle` did
        taken = {m: engs[m].best_info()[2] for m in ("idle", "take")}
        applied = {m: int(eng.opt_state().last_epoch) for m, eng in engs.items()}
        row = {"n_params": n, "step_ms": med, "rounds_ms": rounds, "snapshots": taken, "steps_applied": applied,
               "guards": {m: None if eng.guard is None else eng.guard.cpu().tolist() for m, eng in engs.items()},
               "valid": taken["take"] >= a.takes * a.reps and taken["idle"] == 0,
               "off_spread_ms": max(rounds["off"]) - min(rounds["off"]),
               "idle_minus_off_us": (med["idle"] - med["off"]) * 1e3,
               "take_minus_off_us": (med["take"] - med["off"]) * 1e3,
               "pair_alone_us": {m: pair_alone_us(engs[m], m, 20 * a.reps) for m in ("idle", "take")},
               "take_bytes": 8 * n, "take_bound_us": 8 * n / HBM_PEAK * 1e6, "idle_bytes": 12}
        res["shapes"][shape] = row
        print(f"{shape}: valid {row['valid']} snapshots {taken} applied {applied}  n_params {n}  "
              f"off {med['off']:.4f} ms (spread {row['off_spread_ms'] * 1e3:.1f} us)  "
              f"idle {row['idle_minus_off_us']:+.1f} us  take {row['take_minus_off_us']:+.1f} us  | the pair alone: "
              f"idle {row['pair_alone_us']['idle']:.1f} us, take {row['pair_alone_us']['take']:.1f} us "
              f"({8 * n / 1e6:.1f} MB, bound {row['take_bound_us']:.1f} us at 8 TB/s)", file=sys.stderr, flush=True)
        del engs
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
