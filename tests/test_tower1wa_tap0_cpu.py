"""CPU suite for the trunk kernel's fourth left-out pair, (pixel tile 5, tap 0) (tools/gen_tower1wa.py: SKIP == DEAD under the
product schedule): the generated stream holds no tap-0 product of the file-0 tile, that tile takes the bias row with its
(tap 1, K-step 0) MFMA where the layer has no selector MFMA, and the symbolic checker notices the pair's MFMA coming back
or the bias-taking MFMA going missing."""
import copy
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(ROOT, "tools")
sys.path.insert(0, TOOLS)

NBLOCKS = 3


def _linear(g):
    pro = g.sec_pro(False)
    even = [g.sec_even(False, b) for b in range(NBLOCKS)]
    odd = [g.sec_odd(False, b) for b in range(NBLOCKS)]
    x2 = [g.sec_x2(False, b) for b in range(NBLOCKS)]
    fin = g.sec_fin(False, NBLOCKS - 1)
    lin = [g.Ins("", "blk", blk=0)] + list(pro.ins)
    for b in range(NBLOCKS):
        lin += [g.Ins("", "blk", blk=b)] + even[b].ins + odd[b].ins
        lin += x2[b].ins if b < NBLOCKS - 1 else fin.ins
    return g.insert_lgkm_waits(lin)


@pytest.fixture(scope="module")
def g():
    import gen_tower1wa
    return gen_tower1wa


@pytest.fixture(scope="module")
def checked(g):
    """the linearized 3-block instance, checked once; the tests below only read it"""
    lin = _linear(g)
    assert g.check_and_fill(lin, NBLOCKS)
    return lin


def test_a_clean_environment_leaves_out_the_whole_dead_set():
    env = {k: v for k, v in os.environ.items() if not k.startswith("XQ_1WA_")}
    out = subprocess.run([sys.executable, "-c", "import gen_tower1wa as g; print(sorted(g.SKIP)); print(sorted(g.DEAD))"],
                         cwd=TOOLS, env=env, check=True, capture_output=True, text=True).stdout.split("\n")
    skip, dead = eval(out[0]), eval(out[1])
    assert skip == dead and (5, 0) in skip and len(skip) == 4


def test_stream_has_1600_products_per_layer_and_none_of_tile5_tap0(g, checked):
    assert g.SKIP == g.DEAD and (5, 0) in g.SKIP and len(g.SKIP) == 4
    seen = {}
    for x in checked:
        if x.kind == "mfma" and x.m["want"][0] != "skip":
            key = (x.m["want"][0], x.m["tile"], x.m["want"][1], x.m["want"][2])
            seen[key] = seen.get(key, 0) + 1
    per_layer = {}
    for (layer, _t, _tap, _ks), c in seen.items():
        per_layer[layer] = per_layer.get(layer, 0) + c
    assert per_layer == {layer: 1728 - 32 * 4 for layer in range(2 * NBLOCKS)}
    want = {(layer, t, tap, ks) for layer in range(2 * NBLOCKS) for t in range(48) for tap in range(9) for ks in range(4)
            if (t % 6, tap) not in g.SKIP}
    assert set(seen) == want and set(seen.values()) == {1}
    assert not any(t % 6 == 5 and tap == 0 for (_l, t, tap, _ks) in seen)


def test_first_mfma_of_every_tile_takes_the_bias_row(g, checked):
    """per layer and tile: the first MFMA in stream order is the one and only one emitted with the bias row as C.  With a
    selector MFMA in the layer (a block's second convolution) that is the selector; without, it is (tap 0, K-step 0) for pixel
    tiles 0..4 and (tap 1, K-step 0) for pixel tile 5."""
    by = {}
    for x in checked:
        if x.kind == "mfma":
            w = x.m["want"]
            layer = w[1] if w[0] == "skip" else w[0]
            by.setdefault((layer, x.m["tile"]), []).append(x)
    assert sorted(by) == [(layer, t) for layer in range(2 * NBLOCKS) for t in range(48)]
    for (layer, t), ms in by.items():
        assert ms[0].m["first"] and not any(x.m["first"] for x in ms[1:]), (layer, t)
        has_sel = any(x.m["want"][0] == "skip" for x in ms)
        assert has_sel == bool(layer & 1)
        if has_sel:
            assert ms[0].m["want"] == ("skip", layer), (layer, t)
            conv0 = ms[1].m["want"]
        else:
            conv0 = ms[0].m["want"]
        assert conv0 == ((layer, 1, 0) if t % 6 == 5 else (layer, 0, 0)), (layer, t, conv0)
        # C of the emitted instruction: the bias registers of the weight tile, not the tile itself
        regs = re.findall(r"a\[(\d+):\d+\]", ms[0].text)
        assert int(regs[0]) == 4 * t and int(regs[-1]) == g.A_BIAS + 4 * (t // 6), ms[0].text
        assert all(re.findall(r"a\[(\d+):\d+\]", x.text) == [str(4 * t)] * 2 for x in ms[1:]), (layer, t)


@pytest.mark.parametrize("layer", [2, 3])
def test_the_checker_notices_tile5_tap0_coming_back(g, layer):
    """the left-out pair's MFMA with the operands of its neighbour tile's MFMA of the same K-step: fragments loaded and waited
    for, in (tap, ks) order for its accumulator - wrong only in that the schedule says its pair is left out"""
    lin = _linear(g)
    i = next(i for i, x in enumerate(lin) if x.kind == "mfma" and x.m["tile"] == g.TILE(3, 4) and x.m["want"] == (layer, 0, 0))
    ins = copy.copy(lin[i])
    ins.m = dict(ins.m, tile=g.TILE(3, 5))
    lin.insert(i + 1, ins)
    with pytest.raises(g.CheckError):
        g.check_and_fill(lin, NBLOCKS)


@pytest.mark.parametrize("layer", [0, 2, 3])
def test_the_checker_notices_tile5_losing_tap1_kstep0(g, layer):
    """layers 0 and 2 have no selector MFMA: the deleted one is the tile's bias-taking first MFMA; layer 3 has: a plain product"""
    lin = _linear(g)
    i = next(i for i, x in enumerate(lin) if x.kind == "mfma" and x.m["tile"] == g.TILE(3, 5) and x.m["want"] == (layer, 1, 0))
    del lin[i]
    with pytest.raises(g.CheckError):
        g.check_and_fill(lin, NBLOCKS)


def test_committed_body_leaves_out_the_whole_dead_set():
    text = open(os.path.join(ROOT, "chinesechessai_amd", "csrc", "xq_tower1wa_body.inc")).read()
    dead = re.search(r"^#define XQ_1WA_DEAD_TAPS (\{.*\})$", text, re.M).group(1)
    skip = re.search(r"^#define XQ_1WA_SKIP_TAPS (\{.*\})$", text, re.M).group(1)
    assert skip == dead
    masks = [int(v, 16) for v in re.findall(r"0x[0-9a-f]+", skip)]
    assert masks == [0, 0, 0, 0, 0x004, 0x049]
    # 3,504 MFMA lines per body, plain and stamped
    for name in ("XQ_1WA_BODY", "XQ_1WA_BODY_STAMPED"):
        body = text.split("#define %s \\\n" % name)[1].split('    ""\n')[0]
        assert body.count('"v_mfma_f32_16x16x32_bf16 ') == 3504, name
