"""bench.py --dump-outputs without a GPU: dump_outputs on a synthetic buffer of sample records in the production wire
format (distributed.RECORD_DTYPE) decodes every field, blanks what a record does not define, samples the same games
every time and writes float arrays only."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def test_dump_outputs_decodes_masks_and_samples_by_a_fixed_seed(tmp_path, monkeypatch):
    import bench
    from chinesechessai_amd import distributed as xd
    monkeypatch.setattr(bench, "DUMP_SAMPLE_GAMES", 5)
    monkeypatch.setattr(bench, "DUMP_SCALAR_GAMES", 11)
    G = 23
    rng = np.random.RandomState(1)
    raw = rng.randint(0, 256, size=G * 70 * xd.RECORD_BYTES).astype(np.uint8)         # garbage wherever nothing is defined
    rec = np.frombuffer(raw.tobytes(), dtype=xd.RECORD_DTYPE).reshape(G, 70).copy()
    rec["valid"] = rng.randint(0, 2, size=(G, 70))
    rec["n_moves"] = rng.randint(0, 129, size=(G, 70))
    rec["z"] = rng.standard_normal((G, 70))
    t = torch.from_numpy(np.frombuffer(rec.tobytes(), dtype=np.uint8).copy())
    outcomes = {"n_plies": np.arange(G, dtype=np.int32)}
    dirs = [tmp_path / "a", tmp_path / "b"]
    for d in dirs:
        bench.dump_outputs(str(d), t, G, outcomes)
    a, b = ({f[:-4]: np.load(d / f) for f in sorted(os.listdir(d))} for d in dirs)
    assert sorted(a) == sorted(b)
    for k in a:
        assert a[k].dtype in (np.float32, np.float64) and np.array_equal(a[k], b[k]), k
    gi, si = a["scalar_games"].astype(int), a["sample_games"].astype(int)
    assert len(gi) == 11 and len(si) == 5 and (np.diff(gi) > 0).all() and (np.diff(si) > 0).all()
    valid = rec["valid"][gi] != 0
    assert np.array_equal(a["valid"], valid.astype(np.float32))
    assert a["z"].dtype == np.float64 and np.array_equal(a["z"], np.where(valid, rec["z"][gi], 0.0))
    for k in ("player", "n_moves", "chosen"):
        assert np.array_equal(a[k], np.where(valid, rec[k][gi], 0).astype(np.float32)), k
    assert np.array_equal(a["outcome_n_plies"], np.arange(G, dtype=np.float32))
    for j, g in enumerate(si):
        for p in range(70):
            r = rec[g, p]
            n = int(r["n_moves"]) if r["valid"] else 0
            assert np.array_equal(a["sample_moves"][j, p, :n], r["moves"][:n]) and not a["sample_moves"][j, p, n:].any()
            assert np.array_equal(a["sample_counts"][j, p, :n], r["counts"][:n]) and not a["sample_counts"][j, p, n:].any()
            want = xd.unpack_board(r["board"]).reshape(90) if r["valid"] else np.zeros(90)
            assert np.array_equal(a["sample_board"][j, p], want)
