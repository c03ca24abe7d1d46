"""Host models of two pieces of device bookkeeping, plain NumPy (no GPU), and the slot masks the GPU tests feed them.

number_rows   the evaluator row numbering of k_assign_rows as include/xq_selfplay.h describes it
              (xq_engine_set_row_compaction / xq_engine_set_leaf_dedupe / xq_engine_row_map_net): rows in slot order within
              each network, a duplicate takes the row of its group's lowest slot, a cached or non-pending slot gets -1.
DequeRing     collections.deque(maxlen) for record tags: what xq_replay_push_records promises ("push every valid record
              ... in game / ply order (drop-oldest)").

tests/test_row_model_cpu.py checks both against brute-force loops; tests/test_gpu_row_numbering.py and
tests/test_gpu_replay_push.py compare the kernels with them.
"""
import collections

import numpy as np

PASS = 16 * 1024        # slots k_assign_rows numbers per pass (1,024 threads x 16 slots)
SPAN = 1024             # slots of one wave of a pass (64 lanes x 16 slots): one partial sum of the scan
MAX_PLIES = 70

# the slot counts of the numbering tests: one vector, around a wave span, around one / two / three passes, ragged tails
# (16,401 = one pass + 17, 32,785 = two passes + 17, 49,169 = three passes + 17)
SLOT_COUNTS = (1, 15, 16, 17, 1023, 1024, 1025, 16383, 16384, 16385, 16401, 32785, 49169)
MASK_KINDS = ("all", "alternating", "random50", "random03", "boundaries")
MIXED_KINDS = ("alternating", "random50", "random03")      # families that promise mixed_spans()


def number_rows(pending, net1=None, dup_of=None, cached=None):
    """(leaf_row int32[n], row_src0, row_src1, count0, count1) for n slots.
    pending[s]  the slot holds a pending leaf
    net1[s]     the leaf waits for network 1 (None: single network, everything is network 0's)
    dup_of[s]   leaf dedupe: the lowest slot of the slot's group of equal positions (s itself, or -1, for a slot that is
                its group's lowest / on its own); groups never span networks
    cached[s]   the evaluation cache answers the leaf: it needs no row
    leaf_row[s] = the row inside the slot's own network's buffers or -1; row_srcK[r] = the slot whose planes row r of
    network K reads; rows are numbered in slot order within each network."""
    pending = np.asarray(pending, dtype=bool)
    n = len(pending)
    net = np.zeros(n, bool) if net1 is None else np.asarray(net1, dtype=bool)
    live = pending & ~(np.zeros(n, bool) if cached is None else np.asarray(cached, dtype=bool))
    slots = np.arange(n)
    rep_of = slots.copy() if dup_of is None else np.where(np.asarray(dup_of) < 0, slots, np.asarray(dup_of))
    own = live & (rep_of == slots)
    leaf_row = np.full(n, -1, np.int32)
    src = []
    for k in (False, True):
        idx = np.nonzero(own & (net == k))[0]
        leaf_row[idx] = np.arange(len(idx), dtype=np.int32)
        src.append(idx.astype(np.int32))
    dups = np.nonzero(live & ~own)[0]
    leaf_row[dups] = leaf_row[rep_of[dups]]
    return leaf_row, src[0], src[1], len(src[0]), len(src[1])


def pass_boundaries(n):
    return list(range(PASS, n, PASS))


def _mix(mask, rng):
    """every whole wave span gets at least one live and one dead slot (changes nothing where that already holds)"""
    for s0 in range(0, len(mask) - SPAN + 1, SPAN):
        span = mask[s0:s0 + SPAN]
        if not span.any():
            span[rng.integers(SPAN)] = True
        if span.all():
            span[rng.integers(SPAN)] = False
    return mask


def make_mask(kind, n, seed=0):
    """live[n] of one mask family.  "alternating" and "random*" promise mixed_spans(); "all" and "boundaries" are the two
    extremes on purpose (every partial sum full; every partial sum zero but those at a pass boundary)."""
    rng = np.random.default_rng(1000003 * n + seed)
    if kind == "all":
        return np.ones(n, bool)
    if kind == "alternating":
        return (np.arange(n) & 1) == 0
    if kind == "random50":
        return _mix(rng.random(n) < 0.5, rng)
    if kind == "random03":
        return _mix(rng.random(n) < 0.03, rng)
    if kind == "boundaries":
        # the only live slots: the last of a pass and the first of the next - and the first and the last slot of all, the
        # outer boundaries (so that small counts have a live slot and a ragged tail ends on one)
        m = np.zeros(n, bool)
        for b in pass_boundaries(n):
            m[b - 1] = m[b] = True
        m[0] = m[n - 1] = True
        return m
    raise ValueError(kind)


def mixed_spans(mask):
    """The condition that keeps a case from passing because a boundary carried zero (or a full count): within every
    16,384-slot pass, every 1,024-slot wave span that lies inside the slots holds a live and a dead slot."""
    mask = np.asarray(mask, dtype=bool)
    for s0 in range(0, len(mask) - SPAN + 1, SPAN):          # (spans never straddle a pass: PASS is a multiple of SPAN)
        span = mask[s0:s0 + SPAN]
        if not span.any() or span.all():
            return False
    return True


def dedupe_assignment(n, n_positions, seed=0):
    """(live[n], pos[n]) for the leaf-dedupe cases: position pos[s] in 0 .. n_positions-1 for every slot, such that every
    position's lowest slot lies in pass 0 and every later pass holds further members of it; live promises mixed_spans()."""
    rng = np.random.default_rng(7919 * n + seed)
    live = _mix(rng.random(n) < 0.6, rng)
    pos = rng.integers(0, n_positions, n)
    # by construction, not by luck: slots 1 .. of pass 0 and of every later pass hold every position once, live (slot 0 of
    # each pass is dead: the span keeps a dead slot whatever the draw was)
    for p0 in range(0, n, PASS):
        k = min(n_positions, n - p0 - 1)
        live[p0] = False
        pos[p0 + 1:p0 + 1 + k] = np.arange(k)
        live[p0 + 1:p0 + 1 + k] = True
    return live, pos


def two_network_split(n):
    """net1[n] of the two-network cases: a coin per slot (tests/test_row_model_cpu.py shows that with the random50 mask
    every whole wave span then holds rows of both networks)"""
    rng = np.random.default_rng(31 * n + 5)
    return rng.random(n) < 0.5


def dup_of_groups(live, keys):
    """dup_of for number_rows: keys[s] = anything hashable that names the slot's group (position and network)"""
    first = {}
    dup = np.full(len(live), -1, np.int64)
    for s in np.nonzero(live)[0]:
        dup[s] = first.setdefault(keys[s], int(s))
    return dup


GAP_KINDS = ("first_invalid", "every_second", "hole", "only_last")


def prefix_flags(n_games, seed=0):
    """valid[n_games][70] with ragged prefix lengths 0 .. 70, six games in ten empty (70 and 1 occur)"""
    rng = np.random.default_rng(104729 * n_games + seed)
    length = np.where(rng.random(n_games) < 0.6, 0, rng.integers(1, MAX_PLIES + 1, n_games))
    length[rng.integers(n_games)] = MAX_PLIES
    length[n_games - 1] = 1                                   # the last game is not empty: the scan's last entry counts
    return np.arange(MAX_PLIES)[None, :] < length[:, None]


def gap_flags(n_games, seed=0):
    """prefix_flags with four games in five replaced by a game whose valid flags are NOT a prefix, the four kinds in turn
    (game g with g % 5 < 4): first ply invalid, every second ply, one hole in the middle, only ply 69"""
    valid = prefix_flags(n_games, seed)
    rng = np.random.default_rng(15485863 * n_games + seed)
    for g in range(n_games):
        if g % 5 == 4:
            continue
        kind = GAP_KINDS[g % 5]
        row = np.zeros(MAX_PLIES, bool)
        if kind == "first_invalid":
            row[1:int(rng.integers(2, MAX_PLIES + 1))] = True
        elif kind == "every_second":
            row[int(rng.integers(2))::2] = True
        elif kind == "hole":
            row[:int(rng.integers(10, MAX_PLIES + 1))] = True
            row[int(rng.integers(1, 9))] = False
        else:
            row[MAX_PLIES - 1] = True
        valid[g] = row
    return valid


class DequeRing:
    """collections.deque(maxlen=cap) of record tags.  A record's tag is (first_game + game) * 128 + ply: an integer below
    2^24 for the game counts the tests use, so it survives the float32 value target unchanged."""

    def __init__(self, cap):
        self.cap = int(cap)
        self.items = collections.deque(maxlen=self.cap)

    def __len__(self):
        return len(self.items)

    def push(self, valid, first_game=0):
        """valid[n_games][70]: appends the tag of every valid record in game / ply order - gaps in a game's flags are
        skipped, nothing behind them is dropped - and returns those tags (int64)."""
        valid = np.asarray(valid).astype(bool).reshape(-1, MAX_PLIES)
        g, p = np.nonzero(valid)                              # row-major: game order, ply order
        tags = (g.astype(np.int64) + int(first_game)) * 128 + p
        self.items.extend(tags.tolist())
        return tags

    def tags(self):
        return np.array(self.items, dtype=np.int64)
