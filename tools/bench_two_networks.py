#!/usr/bin/env python3
"""Two-network games in the refill pool against the only way to play the same games without per-slot network
selection: one refill self-play session plus one lock-step opponent play().

Workload (bench.py's play-refill form): --games concurrent slots, --sims simulations, the --blocks-block bf16 network
twice with different seeds (random-init), --total games per configuration:

  all_pairing_1     every game "network A red vs network B black", one refill session
  mixed_50_50       the trainer's epoch (trainer.py:186-209): total // 2 self-play games, the rest A vs B, one refill session
  separate_all_1    the same games as all_pairing_1 in lock-step opponent play() batches of --games (slots of finished
                    games idle until the batch's longest game ends)
  separate_50_50    the same games as mixed_50_50: a refill self-play session of total // 2 games, then lock-step opponent
                    play() batches for the rest
  all_pairing_1_reuse, mixed_50_50_reuse
                    the two one-session configurations with play_refill(reuse=True): root evaluation carry-over in the
                    self-play slots, one evaluation cache for both networks with a three-ply window
                    (SelfPlayEngine.set_per_slot_reuse).  Each gets a fresh pair of evaluators, so the cache's adaptive
                    suspension (a play that answered under 1 % of its rows switches it off for the next 15) is decided
                    by that configuration's own warm-up run; the figure reports what the last timed run did.

--peaked scales both networks' policy_fc.weight and .bias by 256 (bench.py's value_peaked_priors recipe: peaked priors,
a stand-in for trained networks, the regime the cache is for).  --configs a,b,... runs only those.

Prints one JSON line; informational (no threshold).  The games of a one-session run, of its reuse form and of its
separate counterpart are the same games (tests/test_gpu_two_networks.py, tests/test_gpu_two_network_reuse.py), so games/s
compare like for like.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=16384, help="concurrent slots")
    ap.add_argument("--total", type=int, default=0, help="games per configuration (default 2 x --games)")
    ap.add_argument("--sims", type=int, default=50)
    ap.add_argument("--blocks", type=int, default=6)
    ap.add_argument("--repeats", type=int, default=2, help="timed runs per configuration after one warm-up run; the best is reported")
    ap.add_argument("--peaked", action="store_true", help="policy_fc.weight and .bias of both networks x 256 (peaked priors)")
    ap.add_argument("--configs", default="", help="comma-separated subset of the configurations (default: all)")
    args = ap.parse_args()
    import torch
    from chinesechessai_amd import _lib, distributed as xd
    from chinesechessai_amd.engine import SelfPlayEngine, TorchNetEvaluator
    from chinesechessai_amd.neural_network import ChessNet
    G, S = args.games, args.sims
    T = args.total or 2 * G
    if T < 2 * G or T % (2 * G):
        sys.exit("--total must be a multiple of 2 x --games")
    nets = []
    for seed in (0, 1):
        torch.manual_seed(seed)
        nets.append(ChessNet(num_blocks=args.blocks).eval().cuda())
        if args.peaked:
            with torch.no_grad():
                nets[-1].policy_fc.weight.mul_(256.0)
                nets[-1].policy_fc.bias.mul_(256.0)
    evA, evB = TorchNetEvaluator(nets[0]), TorchNetEvaluator(nets[1])
    seeds = np.arange(T, dtype=np.uint32)
    records = torch.zeros(T * _lib.MAX_PLIES * xd.RECORD_BYTES, dtype=torch.uint8, device="cuda")
    eng = SelfPlayEngine(G, sims=S, planes_format=evA.planes_format)
    eng_opp = SelfPlayEngine(G, sims=S, planes_format=evA.planes_format, opponent_mode=True)

    def session(pairing, evs=None):
        a, b = evs or (evA, evB)
        out, plies = eng.play_refill(a, seeds, records.data_ptr(), opponent_evaluator=b, pairing=pairing, reuse=evs is not None)
        return int(out["n_plies"].sum())

    def separate(n_self):
        plies = 0
        if n_self:
            out, _ = eng.play_refill(evA, seeds[:n_self], records.data_ptr())
            plies += int(out["n_plies"].sum())
        for lo in range(n_self, T, G):
            eng_opp.play(evA, seeds[lo:lo + G], opponent_evaluator=evB, read=False)
            eng_opp.pack_samples(records.data_ptr() + lo * _lib.MAX_PLIES * xd.RECORD_BYTES)
            plies += int(eng_opp.read_game_outcomes()["n_plies"].sum())
        return plies

    half = np.zeros(T, np.uint8)
    half[T // 2:] = 1
    configs = [("all_pairing_1", lambda: session(np.ones(T, np.uint8))), ("mixed_50_50", lambda: session(half)),
               ("separate_all_1", lambda: separate(0)), ("separate_50_50", lambda: separate(T // 2))]
    reuse_evs = {}
    for name, pairing in (("all_pairing_1_reuse", np.ones(T, np.uint8)), ("mixed_50_50_reuse", half)):
        def run(name=name, pairing=pairing):
            if name not in reuse_evs:
                reuse_evs[name] = (TorchNetEvaluator(nets[0]), TorchNetEvaluator(nets[1]))
            return session(pairing, reuse_evs[name])
        configs.append((name, run))
    if args.configs:
        want = args.configs.split(",")
        unknown = sorted(set(want) - set(n for n, _ in configs))
        if unknown:
            sys.exit("unknown configuration(s): %s" % ", ".join(unknown))
        configs = [(n, f) for n, f in configs if n in want]
    res = {}
    for name, fn in configs:
        best, plies, times = None, 0, []
        for rep in range(1 + args.repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            plies = fn()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            if rep:
                times.append(dt)
            if rep and (best is None or dt < best):
                best = dt
        res[name] = {"games_per_s": T / best, "seconds": best, "plies_played": plies, "timed_runs_games_per_s": [T / t for t in times]}
        if name in reuse_evs:
            a = reuse_evs[name][0]
            res[name]["carry"] = bool(eng._carry_on)
            res[name]["cache_in_last_run"] = bool(eng.eval_cache)
            if eng.eval_cache and a.eval_cache_last:
                res[name]["cache_hits_fills_rows_last_run"] = [int(x) for x in a.eval_cache_last]
    eng.close()
    eng_opp.close()
    out = {"metric": "two-network self-play games/s (informational)", "slots": G, "games": T, "sims": S, "blocks": args.blocks,
           "peaked": bool(args.peaked), "device": torch.cuda.get_device_name(0), "repeats": args.repeats, "configs": res}

    def ratio(a, b):
        return res[a]["games_per_s"] / res[b]["games_per_s"] if a in res and b in res else None
    out["one_session_over_separate"] = {"all_pairing_1": ratio("all_pairing_1", "separate_all_1"),
                                        "mixed_50_50": ratio("mixed_50_50", "separate_50_50"),
                                        "all_pairing_1_reuse": ratio("all_pairing_1_reuse", "separate_all_1"),
                                        "mixed_50_50_reuse": ratio("mixed_50_50_reuse", "separate_50_50")}
    out["reuse_over_plain_session"] = {"all_pairing_1": ratio("all_pairing_1_reuse", "all_pairing_1"),
                                       "mixed_50_50": ratio("mixed_50_50_reuse", "mixed_50_50")}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
