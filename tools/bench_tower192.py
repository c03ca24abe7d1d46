"""Micro-benchmark of the 192-channel single-launch trunk (csrc/xq_tower192.hip) at 16,384 boards, 6 and 10 blocks (run on
the GPU box), against the two things a user of a 192-channel network could do before it existed:
  (b) "library": the convolutional part of the same InferenceNet on PyTorch's library kernels (what
      allow_library_fallback=True runs for a width without a kernel);
  (c) "padded256": k_tower256 (xq_tower256_nhwc_bf16) on the same folded weights zero-padded to 256 channels.
First, in a process of its own at a small size (37 boards), k_tower192 and the padded k_tower256 must agree to the bound of
tests/test_gpu_tower192.py, 2^-8 * max(1, max|out|) * (2 + blocks); nothing is timed when they do not.  Then every leg is
a process of its own with a time limit, the legs alternate, `--rounds` processes per leg; a process times each depth
`TIMINGS` times, each timing HIP events around `LAUNCHES` launches after 3 warm-up launches of the same shape.  No leg
samples a clock: neither k_tower192 nor k_tower256 reads the shader clock, and the tool does not read the SMI clocks.
A leg that fails ends the measurement.
usage: bench_tower192.py [--boards N] [--rounds R] [--leg-timeout S] [--out profiles/tower192_bench.json]"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LEGS = ("k_tower192", "library", "padded256")
DEPTHS, TIMINGS, LAUNCHES, CHECK_BOARDS = (6, 10), 3, 20, 37


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

    def outputs():
        return torch.empty(G, 2880, device="cuda", dtype=torch.bfloat16), torch.empty(G, 720, device="cuda", dtype=torch.bfloat16)

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

    def hip_trunk(entry, w1, wt, bt, hw, hb, blocks, pv):
        args = (st, planes.data_ptr(), w1.data_ptr(), wt.data_ptr(), bt.data_ptr(), hw.data_ptr(), hb.data_ptr(),
                pv[0].data_ptr(), pv[1].data_ptr(), G, blocks, None, None)
        return lambda: _lib.check(entry(*args))

    def padded(inet, blocks, pv):                                # the same folded weights, zero-padded to 256 channels
        bf = dict(device="cuda", dtype=torch.bfloat16)
        w1 = torch.zeros(9, 256, 16, **bf)
        w1[:, :192] = inet.hip_w[0]
        wt = torch.zeros(2 * blocks, 9, 256, 256, **bf)
        wt[:, :, :192, :192] = inet.hip_wt
        bt = torch.zeros(1 + 2 * blocks, 256, device="cuda", dtype=torch.float32)
        bt[:, :192] = inet.hip_bt
        hw = torch.zeros(64, 256, **bf)
        hw[:, :192] = inet.hip_hw
        keep = (w1, wt, bt, hw)
        return hip_trunk(L.xq_tower256_nhwc_bf16, w1, wt, bt, hw, inet.hip_hb, blocks, pv), keep

    out = {"leg": name, "depths": {}}
    for blocks in DEPTHS:
        torch.manual_seed(blocks)
        net = ChessNet(num_channels=192, num_blocks=blocks).eval().cuda()
        inet = InferenceNet(net)

        def own(pv):
            return hip_trunk(L.xq_tower192_nhwc_bf16, inet.hip_w[0], inet.hip_wt, inet.hip_bt, inet.hip_hw, inet.hip_hb, blocks, pv)
        res = {}
        if name == "check":
            pa, pc = outputs(), outputs()
            own(pa)()
            fn, keep = padded(inet, blocks, pc)
            fn()
            torch.cuda.synchronize()
            res["max_abs_diff_policy_value"] = [float((a.float() - c.float()).abs().max()) for a, c in zip(pa, pc)]
            res["max_abs_output_policy_value"] = [float(a.float().abs().max()) for a in pa]
            res["bound_policy_value"] = [2.0 ** -8 * max(1.0, m) * (2 + blocks) for m in res["max_abs_output_policy_value"]]
            res["ok"] = all(d <= b and m > 0 for d, b, m in zip(res["max_abs_diff_policy_value"], res["bound_policy_value"],
                                                                res["max_abs_output_policy_value"]))
        else:
            if name == "k_tower192":
                fn = own(outputs())
            elif name == "library":
                def fn(lib=inet):                                # InferenceNet.forward's library branch up to the head activations
                    with torch.no_grad():
                        a = F.relu(F.conv2d(x, lib.cw[0], lib.cb[0], padding=1))
                        for i in range(lib.n_blocks):
                            y = F.relu(F.conv2d(a, lib.cw[1 + 2 * i], lib.cb[1 + 2 * i], padding=1))
                            y = F.conv2d(y, lib.cw[2 + 2 * i], lib.cb[2 + 2 * i], padding=1)
                            a = F.relu(y + a)
                        return F.relu(F.conv2d(a, lib.hw, lib.hb))
            else:
                fn, keep = padded(inet, blocks, outputs())
            res["ms_per_launch"] = [round(timeit(fn), 4) for _ in range(TIMINGS)]
        out["depths"][str(blocks)] = res
        del inet, net
        torch.cuda.empty_cache()
    print("LEG " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--boards", type=int, default=16384)
    ap.add_argument("--rounds", type=int, default=3, help="processes per leg, the legs alternating")
    ap.add_argument("--leg-timeout", type=int, default=150, help="seconds one leg's process may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tower192_bench.json"))
    ap.add_argument("--leg", default="", help="(internal) run this one leg in this process")
    args = ap.parse_args()
    if args.leg:
        leg(args.leg, args.boards)
        return
    G = args.boards

    def run_leg(name, boards):
        pr = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", name, "--boards", str(boards)],
                            stdout=subprocess.PIPE, text=True, timeout=args.leg_timeout)
        if pr.returncode != 0:                                   # (nothing more is started behind a leg that failed)
            sys.exit("leg %s failed with status %d" % (name, pr.returncode))
        return json.loads([ln for ln in pr.stdout.splitlines() if ln.startswith("LEG ")][-1][4:])

    check = run_leg("check", CHECK_BOARDS)["depths"]
    print("check", check, flush=True)
    if not all(c["ok"] for c in check.values()):
        sys.exit("k_tower192 and the padded k_tower256 disagree beyond the test's bound: nothing timed")
    runs = {name: [] for name in LEGS}
    for _ in range(args.rounds):
        for name in LEGS:
            runs[name].append(run_leg(name, G))
            print(name, {b: r["ms_per_launch"] for b, r in runs[name][-1]["depths"].items()}, flush=True)
    result = {"boards": G, "processes_per_leg": args.rounds, "timings_per_process": TIMINGS, "launches_per_timing": LAUNCHES,
              "timer": "HIP events around the launches, 3 warm-up launches before each timing",
              "clocks": "not sampled: no leg reads the shader clock and the tool does not read the SMI clocks",
              "flop": "algorithmic: 2*90*(16*9*C + 2*blocks*C*9*C + C*40) per board, C = 192 for every leg",
              "check_at_%d_boards" % CHECK_BOARDS: check, "cases": []}
    for blocks in DEPTHS:
        ms = {name: [t for r in runs[name] for t in r["depths"][str(blocks)]["ms_per_launch"]] for name in LEGS}
        new = ms["k_tower192"]
        case = {"blocks": blocks, "mflop_per_board": flop(1, 192, blocks) / 1e6,
                "ms_per_launch": ms, "ms_spread": {k: round(max(v) - min(v), 4) for k, v in ms.items()},
                "k_tower192_pflops_algorithmic": [round(flop(G, 192, blocks) / max(new) / 1e12, 4), round(flop(G, 192, blocks) / min(new) / 1e12, 4)],
                # the least favourable pairing: the other side's fastest run over k_tower192's slowest
                "library_fastest_over_k_tower192_slowest": round(min(ms["library"]) / max(new), 3),
                "padded256_fastest_over_k_tower192_slowest": round(min(ms["padded256"]) / max(new), 3)}
        result["cases"].append(case)
        print("blocks=%d: library / k_tower192 = %.3f, padded256 / k_tower192 = %.3f (least favourable pairing)" % (
            blocks, case["library_fastest_over_k_tower192_slowest"], case["padded256_fastest_over_k_tower192_slowest"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
