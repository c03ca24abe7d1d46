"""What the MXFP8 single-launch trunk (csrc/xq_tower_mx.hip, k_tower_mx, InferenceNet(trunk="mxfp8")) is worth and how far it
moves the outputs, against the default bf16 trunk (xq_tower_nhwc_bf16: k_tower1wa at these sizes) on the same seeded
128-channel networks (run on the GPU box).  Three parts, each in a fresh child process (the driver never opens the GPU):

  kernel    16,384 boards, 6 and 20 blocks, both kernels alternating in one process: HIP events around 20 launches after 3
            warm-ups, three timings per side; ms, TFLOP/s against the algorithmic count of DESIGN §5, and the least
            favourable pairing of runs (slowest k_tower_mx against fastest k_tower1wa)  -> profiles/tower_mx_bench.json
  selfplay  whole self-play at BASELINE C3's shape (a refill session of --total games through 16,384 slots, 50 simulations,
            6 blocks, random-init weights), trunk="mxfp8" against the default, every leg a process of its own, legs
            alternating, --repeats rounds, a warm-up and a timed session each; games/s of every timed run
  shift     the positions of 1,024 self-play plies (6 blocks, random-init): largest and mean absolute difference of the
            legal-move priors and of the value between the two trunks.  NOT a claim about playing strength.

--channels 256 measures the 256-channel pair instead: k_tower256_mx (csrc/xq_tower256_mx.hip, trunk="mxfp8_256") against
k_tower256 (xq_tower256_nhwc_bf16), the same three parts -> profiles/tower256_mx_bench.json, profiles/tower256_mx_selfplay.json.

usage: bench_tower_mx.py [--channels {128,256}] [--out-kernel profiles/tower_mx_bench.json] [--out profiles/tower_mx_selfplay.json]"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ROUNDS, LAUNCHES = 3, 20
# per width: (trunk value, MX kernel, MX entry point, bf16 kernel, bf16 entry point)
WIDTHS = {128: ("mxfp8", "k_tower_mx", "xq_tower_mxfp8_nhwc", "k_tower1wa", "xq_tower_nhwc_bf16"),
          256: ("mxfp8_256", "k_tower256_mx", "xq_tower256_mxfp8_nhwc", "k_tower256", "xq_tower256_nhwc_bf16")}


def part_kernel(args):
    import torch
    from chinesechessai_amd import _lib
    from chinesechessai_amd.neural_network import ChessNet, InferenceNet
    L, G, C = _lib.lib(), args.games, args.channels
    trunk, mx_name, mx_entry, bf_name, bf_entry = WIDTHS[C]
    mx_fn, bf_fn = getattr(L, mx_entry), getattr(L, bf_entry)
    st = torch.cuda.current_stream().cuda_stream
    torch.manual_seed(0)
    planes = torch.zeros(G, 10, 9, 16, device="cuda", dtype=torch.bfloat16)
    planes[..., :15] = (torch.rand(G, 10, 9, 15, device="cuda") < 0.15).to(torch.bfloat16)
    P = torch.empty(G, 2880, device="cuda", dtype=torch.bfloat16)
    V = torch.empty(G, 720, device="cuda", dtype=torch.bfloat16)

    def flop(blocks):                                           # algorithmic count, padding MFMAs not included
        return 2.0 * G * 90 * (16 * 9 * C + 2 * blocks * C * 9 * C + C * 40)

    def timeit(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for _ in range(3):
            fn()
        e0.record()
        for _ in range(LAUNCHES):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / LAUNCHES

    result = {"boards": G, "launches_per_timing": LAUNCHES, "timings_per_side": ROUNDS, "timer": "HIP events around the launches",
              "flop": "algorithmic: 2*90*(16*9*%d + 2*blocks*%d*9*%d + %d*40) per board" % (C, C, C, C), "cases": []}
    for blocks in (6, 20):
        torch.manual_seed(blocks)
        net = ChessNet(num_channels=C, num_blocks=blocks).eval().cuda()
        ib, im = InferenceNet(net), InferenceNet(net, trunk=trunk)
        head = (ib.hip_hw.data_ptr(), ib.hip_hb.data_ptr(), P.data_ptr(), V.data_ptr(), G, blocks, None, None)
        sides = ((mx_name, lambda: _lib.check(mx_fn(st, planes.data_ptr(), im.hip_w[0].data_ptr(), im.hip_wq.data_ptr(),
                                                    im.hip_ws.data_ptr(), im.hip_bt.data_ptr(), *head))),
                 (bf_name, lambda: _lib.check(bf_fn(st, planes.data_ptr(), ib.hip_w[0].data_ptr(), ib.hip_wt.data_ptr(),
                                                    ib.hip_bt.data_ptr(), *head))))
        ms = {name: [] for name, _ in sides}
        for _ in range(ROUNDS):                                  # alternating
            for name, fn in sides:
                ms[name].append(timeit(fn))
        case = {"blocks": blocks, "sides": {}}
        for name, _ in sides:
            t = ms[name]
            case["sides"][name] = {"ms_per_launch": [round(v, 4) for v in t],
                                   "tflops_algorithmic_best": round(flop(blocks) / min(t) / 1e9, 1)}
        case["%s_fastest_over_%s_slowest" % (bf_name, mx_name)] = round(min(ms[bf_name]) / max(ms[mx_name]), 3)
        result["cases"].append(case)
        del ib, im, net
        torch.cuda.empty_cache()
    print("PART " + json.dumps(result), flush=True)


def part_selfplay(args):
    import numpy as np
    import torch
    from chinesechessai_amd import _lib, distributed as xd
    from chinesechessai_amd.engine import SelfPlayEngine, TorchNetEvaluator
    from chinesechessai_amd.neural_network import ChessNet
    G, T = args.games, args.total
    torch.manual_seed(0)
    net = ChessNet(num_channels=args.channels, num_blocks=6).eval().cuda()
    ev = TorchNetEvaluator(net, eval_cache="on", trunk=args.trunk)    # (no adaptive suspension: both legs run the same machinery)
    eng = SelfPlayEngine(G, sims=50, planes_format=ev.planes_format)
    records = torch.zeros(T * _lib.MAX_PLIES * xd.RECORD_BYTES, dtype=torch.uint8, device="cuda")
    seeds = np.arange(T, dtype=np.uint32)
    for rep in range(2):                                       # warm-up, then the timed session
        eng.row_history(cap=0, reset=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out, _ = eng.play_refill(ev, seeds, records.data_ptr())
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
    rows = eng.row_history()[0]
    res = {"trunk": args.trunk, "seconds": dt, "games_per_s": T / dt, "plies_per_s": int(out["n_plies"].sum()) / dt,
           "rows_per_game": float(rows.astype(np.int64).sum()) / T, "errors": int(out["error"].sum())}
    eng.close()
    print("PART " + json.dumps(res), flush=True)


def part_shift(args):
    import numpy as np
    import torch
    from chinesechessai_amd.engine import SelfPlayEngine, TorchNetEvaluator
    from chinesechessai_amd.neural_network import ChessNet, InferenceNet
    torch.manual_seed(0)
    net = ChessNet(num_channels=args.channels, num_blocks=6).eval().cuda()
    ev = TorchNetEvaluator(net)
    eng = SelfPlayEngine(64, sims=16, planes_format=ev.planes_format, max_moves=16)     # 64 games x 16 plies
    b = eng.play(ev, np.arange(64, dtype=np.uint32))
    eng.close()
    pos = [(g, i) for g in range(64) for i in range(int(b.n_samples[g]))][:1024]
    enc = np.stack([ChessNet.encode_board(b.s_board[g, i].reshape(10, 9), 1 if i % 2 == 0 else -1) for g, i in pos])
    planes = torch.zeros(len(pos), 10, 9, 16, dtype=torch.bfloat16, device="cuda")
    planes[..., :15] = torch.from_numpy(enc).permute(0, 2, 3, 1).to(device="cuda", dtype=torch.bfloat16)
    x = planes.permute(0, 3, 1, 2)
    outs = []
    for trunk in ("bf16", WIDTHS[args.channels][0]):
        inet = InferenceNet(net, trunk=trunk)
        logits, values = inet(x)
        outs.append((logits.float().cpu().numpy().astype(np.float64), values.float().cpu().numpy().astype(np.float64), inet.column_map))
    dp = []
    for k, (g, i) in enumerate(pos):
        cols = outs[0][2][b.s_moves[g, i, :int(b.s_n[g, i])].astype(np.int64)]
        pr = []
        for lg, _, _ in outs:
            z = np.exp(lg[k, cols] - lg[k, cols].max())
            pr.append(z / z.sum())
        dp.append(np.abs(pr[0] - pr[1]))
    dp, dv = np.concatenate(dp), np.abs(outs[0][1] - outs[1][1])
    print("PART " + json.dumps({"positions": len(pos), "legal_moves": int(len(dp)), "prior_abs_diff_max": float(dp.max()),
                                "prior_abs_diff_mean": float(dp.mean()), "prior_mean": float(1.0 / (len(dp) / len(pos))),
                                "value_abs_diff_max": float(dv.max()), "value_abs_diff_mean": float(dv.mean()),
                                "value_abs_mean_bf16": float(np.abs(outs[0][1]).mean()),
                                "note": "6-block random-init network; no claim about playing strength"}), flush=True)


def child(args, part, *extra):
    cmd = [sys.executable, os.path.abspath(__file__), "--part", part, "--games", str(args.games), "--total", str(args.total),
           "--channels", str(args.channels)] + list(extra)
    pr = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=args.part_timeout)
    if pr.returncode != 0:                                   # (a part that failed ends the measurement: nothing more is started)
        sys.exit("part %s %s failed with status %d" % (part, " ".join(extra), pr.returncode))
    return json.loads([ln for ln in pr.stdout.splitlines() if ln.startswith("PART ")][-1][5:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=16384, help="boards per launch / concurrent slots")
    ap.add_argument("--total", type=int, default=32768, help="games per self-play session")
    ap.add_argument("--repeats", type=int, default=2, help="rounds of alternating self-play processes")
    ap.add_argument("--part-timeout", type=int, default=400, help="seconds one child process may take")
    ap.add_argument("--channels", type=int, choices=(128, 256), default=128, help="network width: which pair of kernels")
    ap.add_argument("--out-kernel", default=None, help="default: profiles/tower_mx_bench.json (256: tower256_mx_bench.json)")
    ap.add_argument("--out", default=None, help="default: profiles/tower_mx_selfplay.json (256: tower256_mx_selfplay.json)")
    ap.add_argument("--part", default="", help="(internal) run this one part in this process")
    ap.add_argument("--trunk", default="bf16", help="(internal) the self-play leg")
    args = ap.parse_args()
    if args.part:
        {"kernel": part_kernel, "selfplay": part_selfplay, "shift": part_shift}[args.part](args)
        return
    trunk, mx_name, _, bf_name, _ = WIDTHS[args.channels]
    stem = "tower_mx" if args.channels == 128 else "tower256_mx"
    args.out_kernel = args.out_kernel or os.path.join(ROOT, "profiles", stem + "_bench.json")
    args.out = args.out or os.path.join(ROOT, "profiles", stem + "_selfplay.json")
    kernel = child(args, "kernel")
    with open(args.out_kernel, "w") as f:
        json.dump(kernel, f, indent=1)
        f.write("\n")
    for c in kernel["cases"]:
        print("kernel blocks=%d: %s  fastest %s / slowest %s = %.3f" % (
            c["blocks"], {k: v["ms_per_launch"] for k, v in c["sides"].items()}, bf_name, mx_name,
            c["%s_fastest_over_%s_slowest" % (bf_name, mx_name)]), flush=True)
    runs = {"bf16": [], trunk: []}
    for rnd in range(args.repeats):
        for trunk in runs:
            runs[trunk].append(child(args, "selfplay", "--trunk", trunk))
            print("self-play round %d %s: %.1f games/s" % (rnd, trunk, runs[trunk][-1]["games_per_s"]), flush=True)
    gps = {t: [r["games_per_s"] for r in runs[t]] for t in runs}
    out = {"selfplay": {"slots": args.games, "games": args.total, "sims": 50, "blocks": 6, "runs": runs, "games_per_s": gps,
                        "mxfp8_slowest_over_bf16_fastest": min(gps[trunk]) / max(gps["bf16"]),
                        "mxfp8_best_over_bf16_best": max(gps[trunk]) / max(gps["bf16"])},
           "shift": child(args, "shift")}
    print(json.dumps(out), flush=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
