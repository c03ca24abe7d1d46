#!/usr/bin/env python3
"""What playout cap randomization buys (SelfPlayEngine.set_playout_cap): a refill session of --total games through --games
slots - BASELINE C3's shape: 16,384 slots, 50 simulations, the 6-block bf16 network, random-init weights (and with
--peaked: policy_fc x 256, bench.py's stand-in for a trained network) - once without the cap and once per --legs entry
"full_prob:fast_sims".

Every leg runs in a process of its own (a fresh child each: the driver never opens the GPU), legs alternating, --repeats
rounds; a child plays one warm-up session and one timed session, and the best round of a leg is reported:

  games_per_s, plies_per_s      whole games and plies (searched positions) per second of the timed session
  policy_records_per_s          records with valid = 1 per second: the fully searched plies, what the trainer's policy
                                head is fed (without the cap: every ply)
  rows_per_game                 network rows the evaluator ran, per game (row compaction's count: after the carry-over,
                                the leaf dedupe and the evaluation cache)
  search_round_us               mean of k_search_round from HIP events around every 4th launch

Prints one JSON line; --out writes it to a file too.  Informational: no threshold, and nothing here says whether a capped
run trains a stronger network per GPU-hour.

  python tools/bench_playout_cap.py [--peaked] [--out profiles/playout_cap_bench.json]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
VALID_OFFSET = 48 + 8 + 1 + 1                 # xq_sample_record: board[12], z, player, n_moves, then valid


def run_leg(args, leg):
    import numpy as np
    import torch
    from chinesechessai_amd import _lib, distributed as xd
    from chinesechessai_amd.engine import SelfPlayEngine, TorchNetEvaluator
    from chinesechessai_amd.neural_network import ChessNet
    G, T, S = args.games, args.total, args.sims
    torch.manual_seed(0)
    net = ChessNet(num_blocks=args.blocks).eval().cuda()
    if args.peaked:
        with torch.no_grad():
            net.policy_fc.weight.mul_(256.0)
            net.policy_fc.bias.mul_(256.0)
    ev = TorchNetEvaluator(net, eval_cache="on")          # (no adaptive suspension: every leg runs the same machinery)
    eng = SelfPlayEngine(G, sims=S, planes_format=ev.planes_format)
    if leg != "off":
        p, fast = leg.split(":")
        eng.set_playout_cap(float(p), int(fast), seed=args.cap_seed)
    records = torch.zeros(T * _lib.MAX_PLIES * xd.RECORD_BYTES, dtype=torch.uint8, device="cuda")
    seeds = np.arange(T, dtype=np.uint32)
    res = None
    for rep in range(2):                                   # warm-up, then the timed session
        eng.row_history(cap=0, reset=True)
        eng.profile(4 if rep else 0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out, steps = eng.play_refill(ev, seeds, records.data_ptr())
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if rep:
            prof = eng.profile_read()
            rows, n_rounds = eng.row_history()
            plies = int(out["n_plies"].sum())
            valid = int(records.view(-1, xd.RECORD_BYTES)[:, VALID_OFFSET].to(torch.int64).sum().item())
            res = {"leg": leg, "seconds": dt, "games_per_s": T / dt, "plies_per_s": plies / dt, "policy_records_per_s": valid / dt,
                   "plies": plies, "policy_records": valid, "rows_per_game": float(rows.astype(np.int64).sum()) / T,
                   "rounds_launched": int(n_rounds), "rounds_in_history": int(len(rows)), "steps": int(steps),
                   "search_round_us": 1e3 * prof["search_ms"] / max(prof["search_launches"], 1),
                   "search_rounds_timed": int(prof["search_launches"]), "errors": int(out["error"].sum()),
                   "carry": bool(eng._carry_on), "cache": bool(eng.eval_cache), "dedupe": bool(eng.leaf_dedupe),
                   "device": torch.cuda.get_device_name(0)}
    eng.close()
    print("LEG " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=16384, help="concurrent slots")
    ap.add_argument("--total", type=int, default=32768, help="games per session")
    ap.add_argument("--sims", type=int, default=50)
    ap.add_argument("--blocks", type=int, default=6)
    ap.add_argument("--peaked", action="store_true", help="policy_fc.weight and .bias x 256 (peaked priors)")
    ap.add_argument("--legs", default="0.25:16,0.5:16", help="comma-separated full_prob:fast_sims legs beside the cap-off leg")
    ap.add_argument("--cap-seed", type=int, default=0)
    ap.add_argument("--repeats", type=int, default=2, help="rounds of alternating processes; the best of a leg is reported")
    ap.add_argument("--leg-timeout", type=int, default=400, help="seconds one leg's process may take")
    ap.add_argument("--out", default="")
    ap.add_argument("--leg", default="", help="(internal) run this one leg in this process")
    args = ap.parse_args()
    if args.leg:
        run_leg(args, args.leg)
        return
    legs = ["off"] + [x for x in args.legs.split(",") if x]
    runs = {leg: [] for leg in legs}
    for rnd in range(args.repeats):
        for leg in legs:
            cmd = [sys.executable, os.path.abspath(__file__), "--leg", leg, "--games", str(args.games), "--total", str(args.total),
                   "--sims", str(args.sims), "--blocks", str(args.blocks), "--cap-seed", str(args.cap_seed)]
            if args.peaked:
                cmd.append("--peaked")
            pr = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=args.leg_timeout)
            if pr.returncode != 0:                       # (a leg that failed ends the measurement: nothing more is started)
                sys.exit("leg %s failed with status %d" % (leg, pr.returncode))
            line = [ln for ln in pr.stdout.splitlines() if ln.startswith("LEG ")][-1]
            runs[leg].append(json.loads(line[4:]))
            print("round %d leg %s: %.1f games/s" % (rnd, leg, runs[leg][-1]["games_per_s"]), file=sys.stderr, flush=True)
    res = {}
    for leg in legs:
        best = min(runs[leg], key=lambda r: r["seconds"])
        best["timed_runs_games_per_s"] = [r["games_per_s"] for r in runs[leg]]
        res[leg] = best
    out = {"metric": "playout cap: refill self-play, games/s and policy records/s (informational)", "slots": args.games,
           "games": args.total, "sims": args.sims, "blocks": args.blocks, "peaked": bool(args.peaked), "repeats": args.repeats,
           "legs": res,
           "over_cap_off": {leg: {k: res[leg][k] / res["off"][k] for k in ("games_per_s", "plies_per_s", "policy_records_per_s",
                                                                            "rows_per_game", "search_round_us")}
                            for leg in legs if leg != "off"}}
    text = json.dumps(out)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
