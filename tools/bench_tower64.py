"""Micro-benchmark of the 64-channel single-launch trunk (csrc/xq_tower64.hip) at 16,384 boards, 6 and 10 blocks (run on
the GPU box), against the two things a user of a 64-channel network could do before it existed:
  (a) "library": the convolutional part of the same InferenceNet on PyTorch's library kernels (what
      allow_library_fallback=True runs for a width without a kernel);
  (b) "padded128": k_tower1wa (xq_tower_nhwc_bf16, variant 60) on the same folded weights zero-padded to 128 channels.
Every leg is a process of its own with a time limit, the legs alternate, `--rounds` processes per leg; a process times
each depth `TIMINGS` times, each timing HIP events around `LAUNCHES` launches after 3 warm-up launches.  The padded leg
also reads the shader clock k_tower1wa samples (xq_debug.h) in a pass of its own behind the timings, and the largest
difference between its outputs and k_tower64's on the same planes.  A leg that fails ends the measurement.
usage: bench_tower64.py [--boards N] [--rounds R] [--leg-timeout S] [--out profiles/tower64_bench.json]"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LEGS = ("k_tower64", "library", "padded128")
DEPTHS, TIMINGS, LAUNCHES = (6, 10), 3, 50


def flop(boards, channels, blocks):                             # algorithmic count, padding MFMAs not included
    return 2.0 * boards * 90 * (16 * 9 * channels + 2 * blocks * channels * 9 * channels + channels * 40)


def leg(name, G):
    import torch
    import torch.nn.functional as F
    from chinesechessai_amd import _lib
    from chinesechessai_amd.neural_network import ChessNet, InferenceNet
    L = _lib.lib()
    st = torch.cuda.current_stream().cuda_stream
    torch.manual_seed(0)
    planes = torch.zeros(G, 10, 9, 16, device="cuda", dtype=torch.bfloat16)
    planes[..., :15] = (torch.rand(G, 10, 9, 15, device="cuda") < 0.15).to(torch.bfloat16)
    x = planes.permute(0, 3, 1, 2)                               # logical NCHW, channels-last strides
    P = torch.empty(G, 2880, device="cuda", dtype=torch.bfloat16)
    V = torch.empty(G, 720, device="cuda", dtype=torch.bfloat16)

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

    def hip_trunk(entry, w1, wt, bt, hw, hb, blocks, p=P, v=V):
        args = (st, planes.data_ptr(), w1.data_ptr(), wt.data_ptr(), bt.data_ptr(), hw.data_ptr(), hb.data_ptr(),
                p.data_ptr(), v.data_ptr(), G, blocks, None, None)
        return lambda: _lib.check(entry(*args))

    out = {"leg": name, "depths": {}}
    for blocks in DEPTHS:
        torch.manual_seed(blocks)
        net = ChessNet(num_channels=64, num_blocks=blocks).eval().cuda()
        inet = InferenceNet(net)
        res = {}
        if name == "k_tower64":
            fn = hip_trunk(L.xq_tower64_nhwc_bf16, inet.hip_w[0], inet.hip_wt, inet.hip_bt, inet.hip_hw, inet.hip_hb, blocks)
        elif name == "library":
            def fn(lib=inet):                                    # InferenceNet.forward's library branch up to the head activations
                with torch.no_grad():
                    a = F.relu(F.conv2d(x, lib.cw[0], lib.cb[0], padding=1))
                    for i in range(lib.n_blocks):
                        y = F.relu(F.conv2d(a, lib.cw[1 + 2 * i], lib.cb[1 + 2 * i], padding=1))
                        y = F.conv2d(y, lib.cw[2 + 2 * i], lib.cb[2 + 2 * i], padding=1)
                        a = F.relu(y + a)
                    return F.relu(F.conv2d(a, lib.hw, lib.hb))
        else:
            bf = dict(device="cuda", dtype=torch.bfloat16)
            w1 = torch.zeros(9, 128, 16, **bf)
            w1[:, :64] = inet.hip_w[0]
            wt = torch.zeros(2 * blocks, 9, 128, 128, **bf)
            wt[:, :, :64, :64] = inet.hip_wt
            bt = torch.zeros(1 + 2 * blocks, 128, device="cuda", dtype=torch.float32)
            bt[:, :64] = inet.hip_bt
            hw = torch.zeros(64, 128, **bf)
            hw[:, :64] = inet.hip_hw
            L.xq_tower_set_variant(60)                           # k_tower1wa
            fn = hip_trunk(L.xq_tower_nhwc_bf16, w1, wt, bt, hw, inet.hip_hb, blocks)
        res["ms_per_launch"] = [round(timeit(fn), 4) for _ in range(TIMINGS)]
        if name == "padded128":                                  # behind the timings: clock sample, then the outputs compared
            clock = torch.zeros(3, dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()
            L.xq_tower_set_clock_sample(clock.data_ptr())
            try:
                for _ in range(LAUNCHES):
                    fn()
                torch.cuda.synchronize()
            finally:
                L.xq_tower_set_clock_sample(None)
            clk = clock.cpu().numpy()
            res["k_tower1wa_clock_ghz"] = round(float(clk[0]) / float(clk[1]) * 0.1, 3) if clk[1] > 0 else None
            P64, V64 = torch.empty_like(P), torch.empty_like(V)
            hip_trunk(L.xq_tower64_nhwc_bf16, inet.hip_w[0], inet.hip_wt, inet.hip_bt, inet.hip_hw, inet.hip_hb, blocks, P64, V64)()
            torch.cuda.synchronize()
            res["max_abs_diff_to_k_tower64"] = [float((P.float() - P64.float()).abs().max()), float((V.float() - V64.float()).abs().max())]
            res["max_abs_output"] = [float(P64.float().abs().max()), float(V64.float().abs().max())]
            L.xq_tower_set_variant(-1)
        out["depths"][str(blocks)] = res
        del inet, net
        torch.cuda.empty_cache()
    print("LEG " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--boards", type=int, default=16384)
    ap.add_argument("--rounds", type=int, default=3, help="processes per leg, the legs alternating")
    ap.add_argument("--leg-timeout", type=int, default=150, help="seconds one leg's process may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tower64_bench.json"))
    ap.add_argument("--leg", default="", help="(internal) run this one leg in this process")
    args = ap.parse_args()
    if args.leg:
        leg(args.leg, args.boards)
        return
    G = args.boards
    runs = {name: [] for name in LEGS}
    for _ in range(args.rounds):
        for name in LEGS:
            pr = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", name, "--boards", str(G)],
                                stdout=subprocess.PIPE, text=True, timeout=args.leg_timeout)
            if pr.returncode != 0:                               # (nothing more is started behind a leg that failed)
                sys.exit("leg %s failed with status %d" % (name, pr.returncode))
            runs[name].append(json.loads([ln for ln in pr.stdout.splitlines() if ln.startswith("LEG ")][-1][4:]))
            print(name, {b: r["ms_per_launch"] for b, r in runs[name][-1]["depths"].items()}, flush=True)
    result = {"boards": G, "processes_per_leg": args.rounds, "timings_per_process": TIMINGS, "launches_per_timing": LAUNCHES,
              "timer": "HIP events around the launches, 3 warm-up launches before each timing",
              "flop": "algorithmic: 2*90*(16*9*C + 2*blocks*C*9*C + C*40) per board, C = 64 for every leg", "cases": []}
    for blocks in DEPTHS:
        ms = {name: [t for r in runs[name] for t in r["depths"][str(blocks)]["ms_per_launch"]] for name in LEGS}
        pad = [r["depths"][str(blocks)] for r in runs["padded128"]]
        new = ms["k_tower64"]
        case = {"blocks": blocks, "mflop_per_board": flop(1, 64, blocks) / 1e6,
                "ms_per_launch": ms, "ms_spread": {k: round(max(v) - min(v), 4) for k, v in ms.items()},
                "k_tower64_tflops_algorithmic": [round(flop(G, 64, blocks) / max(new) / 1e9, 1), round(flop(G, 64, blocks) / min(new) / 1e9, 1)],
                # the least favourable pairing: the other side's fastest run over k_tower64's slowest
                "library_fastest_over_k_tower64_slowest": round(min(ms["library"]) / max(new), 3),
                "padded128_fastest_over_k_tower64_slowest": round(min(ms["padded128"]) / max(new), 3),
                "k_tower1wa_clock_ghz": [p["k_tower1wa_clock_ghz"] for p in pad],
                "padded128_max_abs_diff_to_k_tower64_policy_value": pad[0]["max_abs_diff_to_k_tower64"],
                "max_abs_output_policy_value": pad[0]["max_abs_output"]}
        result["cases"].append(case)
        print("blocks=%d: library / k_tower64 = %.3f, padded128 / k_tower64 = %.3f (least favourable pairing)" % (
            blocks, case["library_fastest_over_k_tower64_slowest"], case["padded128_fastest_over_k_tower64_slowest"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
