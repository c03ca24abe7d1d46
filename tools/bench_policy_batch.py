"""Batch formation with the policy target + legal-move loss, device path against the host path a user had before.

Ring: 1,024 games x up to 70 records from one SelfPlayEngine run (HashNet evaluator).  For B = 64 and 4,096, median of 20
after 3 warm-ups, every repetition ended by a stream synchronisation:
  (a) ReplayBuffer.sample_policy_tensors + training.policy_loss forward + backward (everything stays in HBM);
  (b) ReplayBuffer.sample() -> dense float32 [B, 8100] target built on the host from the move_probs dicts -> H2D ->
      dense cross-entropy over the legal mask with torch ops, forward + backward.
Both produce the gradient of the same loss with respect to the same float32 logits [B, 8100].  The backward kernel is
also timed alone (HIP events) and its stored bytes set against 8 TB/s.
usage: python tools/bench_policy_batch.py [--out profiles/policy_batch_bench.json] [--games 1024] [--sims 16]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_HBM = 8.0e12


def timed(fn, reps=20, warm=3):
    import torch
    out = []
    for i in range(warm + reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.current_stream().synchronize()
        if i >= warm:
            out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out), min(out), max(out)


def main():
    import torch
    from chinesechessai_amd import _lib, training
    from chinesechessai_amd import distributed as xd
    from chinesechessai_amd.chess_env import encode_move
    from chinesechessai_amd.engine import HashNetEvaluator, SelfPlayEngine
    from chinesechessai_amd.replay import ReplayBuffer
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "policy_batch_bench.json"))
    ap.add_argument("--games", type=int, default=1024)
    ap.add_argument("--sims", type=int, default=16)
    args = ap.parse_args()

    G = args.games
    eng = SelfPlayEngine(G, sims=args.sims)
    eng.play(HashNetEvaluator(), np.arange(G, dtype=np.uint32), read=False)
    rec = torch.zeros(G * _lib.MAX_PLIES * xd.RECORD_BYTES, dtype=torch.uint8, device="cuda")
    eng.pack_samples(rec.data_ptr())
    eng.close()
    buf = ReplayBuffer(max_size=G * _lib.MAX_PLIES)
    n_rec = buf.push_records(rec, G)
    props = torch.cuda.get_device_properties(0)
    res = {"device": props.name, "clock_rate_khz": getattr(props, "clock_rate", None), "ring_records": int(n_rec),
           "games": G, "sims": args.sims, "n_cols": 8100, "reps": 20, "warmups": 3, "unit": "ms", "batches": {}}

    for B in (64, 4096):
        logits = torch.randn(B, 8100, device="cuda", requires_grad=True)
        rng = np.random.RandomState(B)
        idx = rng.choice(n_rec, B, replace=False)

        def device_path():
            _, _, target = buf.sample_policy_tensors(B, indices=idx)
            logits.grad = None
            training.policy_loss(logits, target).backward()

        def host_path():
            _, probs, _ = buf.sample(B, indices=idx)
            dense = np.zeros((B, 8100), np.float32)
            for b, mp in enumerate(probs):
                for mv, p in mp.items():
                    dense[b, encode_move(mv)] = p
            t = torch.from_numpy(dense).cuda()
            mask = t > 0                                                      # (0 * log 0 must weigh nothing)
            logits.grad = None
            # legal mask = every stored move of the sample, those with probability zero included
            lm = np.zeros((B, 8100), bool)
            for b, mp in enumerate(probs):
                lm[b, [encode_move(mv) for mv in mp]] = True
            legal = torch.from_numpy(lm).cuda()
            logp = torch.log_softmax(logits.masked_fill(~legal, float("-inf")), dim=1)
            loss = -(t * logp.masked_fill(~mask, 0.0)).sum(dim=1).mean()
            loss.backward()

        a = timed(device_path)
        ga = logits.grad.detach().clone()
        b = timed(host_path)
        gb = logits.grad.detach().clone()
        # the backward kernel alone
        _, _, target = buf.sample_policy_tensors(B, indices=idx)
        _, resid = training.policy_loss_rows(logits.detach(), target)
        grad = torch.empty(B, 8100, device="cuda")
        s = torch.cuda.current_stream().cuda_stream
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ks = []
        for i in range(23):
            ev[0].record()
            _lib.lib().xq_policy_loss_grad_f32(C.c_void_p(s), C.c_void_p(resid.data_ptr()), C.c_void_p(target.cols.data_ptr()),
                                               C.c_void_p(target.n_moves.data_ptr()), None, 1.0 / B, B,
                                               C.c_void_p(grad.data_ptr()), 8100, 8100)
            ev[1].record()
            ev[1].synchronize()
            if i >= 3:
                ks.append(ev[0].elapsed_time(ev[1]))
        stored = B * 8100 * 4
        k_ms = statistics.median(ks)
        res["batches"][str(B)] = {
            "device_path_ms": {"median": a[0], "min": a[1], "max": a[2]},
            "host_path_ms": {"median": b[0], "min": b[1], "max": b[2]},
            "host_over_device": b[0] / a[0],
            "max_abs_gradient_difference": float((ga - gb).abs().max()),
            "backward_kernel": {"median_ms": k_ms, "stored_bytes": stored, "ms_at_8TBps": stored / PEAK_HBM * 1e3,
                                "achieved_GBps": stored / (k_ms * 1e-3) / 1e9, "frac_of_8TBps": stored / (k_ms * 1e-3) / PEAK_HBM},
        }
    buf.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
