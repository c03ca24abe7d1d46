"""Micro-benchmark of the 256-channel single-launch trunk (csrc/xq_tower256.hip) at 16,384 boards, 6 and 20 blocks
(run on the GPU box).  In the same process, alternating, two yardsticks: (a) k_tower16b<4> (variant 39) on a 128-channel
network of the same depth - the same MFMA shape and issue style at a quarter of the work per layer - and (b) the
convolutional part of a 256-channel InferenceNet on PyTorch's library kernels, the only way to run this width before.
Every side is timed `rounds` times, so the spread between two runs of a side stands beside the difference between sides.
usage: bench_tower256.py [boards] [output json]"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F
from chinesechessai_amd import _lib
from chinesechessai_amd.neural_network import ChessNet, InferenceNet

L = _lib.lib()
G = int(sys.argv[1]) if len(sys.argv) > 1 else 16384
OUT = sys.argv[2] if len(sys.argv) > 2 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                         "tower256_bench.json")
ROUNDS, LAUNCHES = 3, 20
st = torch.cuda.current_stream().cuda_stream
torch.manual_seed(0)
planes = torch.zeros(G, 10, 9, 16, device="cuda", dtype=torch.bfloat16)
planes[..., :15] = (torch.rand(G, 10, 9, 15, device="cuda") < 0.15).to(torch.bfloat16)
x = planes.permute(0, 3, 1, 2)                                   # logical NCHW, channels-last strides
P = torch.empty(G, 2880, device="cuda", dtype=torch.bfloat16)
V = torch.empty(G, 720, device="cuda", dtype=torch.bfloat16)


def flop(channels, blocks):                                     # algorithmic count, padding MFMAs not included
    return 2.0 * G * 90 * (16 * 9 * channels + 2 * blocks * channels * 9 * channels + channels * 40)


def timeit(fn, it=LAUNCHES):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(3):
        fn()
    e0.record()
    for _ in range(it):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / it


def hip_trunk(inet, entry):
    args = (st, planes.data_ptr(), inet.hip_w[0].data_ptr(), inet.hip_wt.data_ptr(), inet.hip_bt.data_ptr(),
            inet.hip_hw.data_ptr(), inet.hip_hb.data_ptr(), P.data_ptr(), V.data_ptr(), G, inet.n_blocks, None, None)
    return lambda: entry(*args)


def library_trunk(inet):
    """InferenceNet.forward's library branch up to the head activations (MIOpen / hipBLASLt through F.conv2d)."""
    def run():
        with torch.no_grad():
            a = F.relu(F.conv2d(x, inet.cw[0], inet.cb[0], padding=1))
            for i in range(inet.n_blocks):
                y = F.relu(F.conv2d(a, inet.cw[1 + 2 * i], inet.cb[1 + 2 * i], padding=1))
                y = F.conv2d(y, inet.cw[2 + 2 * i], inet.cb[2 + 2 * i], padding=1)
                a = F.relu(y + a)
            return F.relu(F.conv2d(a, inet.hw, inet.hb))
    return run


result = {"boards": G, "launches_per_timing": LAUNCHES, "timings_per_side": ROUNDS, "timer": "HIP events around the launches",
          "flop": "algorithmic: 2*90*(16*9*C + 2*blocks*C*9*C + C*40) per board", "cases": []}
for blocks in (6, 20):
    i256 = InferenceNet(ChessNet(num_channels=256, num_blocks=blocks).eval().cuda())
    i128 = InferenceNet(ChessNet(num_channels=128, num_blocks=blocks).eval().cuda())
    L.xq_tower_set_variant(39)
    sides = (("k_tower256", hip_trunk(i256, L.xq_tower256_nhwc_bf16), flop(256, blocks)),
             ("k_tower16b<4>, 128 channels", hip_trunk(i128, L.xq_tower_nhwc_bf16), flop(128, blocks)),
             ("library kernels, 256 channels", library_trunk(i256), flop(256, blocks)))
    ms = {name: [] for name, _, _ in sides}
    for _ in range(ROUNDS):                                      # alternating
        for name, fn, _ in sides:
            ms[name].append(timeit(fn))
    L.xq_tower_set_variant(-1)
    case = {"blocks": blocks, "gflop_per_board_256": flop(256, blocks) / G / 1e9, "sides": {}}
    for name, _, fl in sides:
        t = ms[name]
        case["sides"][name] = {"ms_per_launch": [round(v, 4) for v in t], "ms_spread": round(max(t) - min(t), 4),
                               "tflops_algorithmic_best": round(fl / min(t) / 1e9, 1)}
        print("%s G=%d blocks=%d: %s ms  best %.1f TFLOP/s (algorithmic)" % (name, G, blocks, ["%.3f" % v for v in t], fl / min(t) / 1e9))
    new, lib = ms["k_tower256"], ms["library kernels, 256 channels"]
    case["library_over_k_tower256"] = round(min(lib) / max(new), 3)          # the least favourable pairing of runs
    case["faster_than_library_beyond_spread"] = bool(min(lib) - max(new) > max(max(new) - min(new), max(lib) - min(lib)))
    result["cases"].append(case)
    del i256, i128
    torch.cuda.empty_cache()
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
with open(OUT, "w") as f:
    json.dump(result, f, indent=1)
    f.write("\n")
print("wrote", OUT)
