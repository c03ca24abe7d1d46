"""Host mirror of trainer.py's ReplayBuffer (trainer.py:22-44) on a device-resident ring.

    buf = ReplayBuffer(max_size=10000)
    buf.push_records(records_tensor, n_games)     # engine.pack_samples() / all-gathered shards
    buf.push(game_data)                           # reference-format [(board, {move: p}, z)] tuples
    states, targets = buf.sample_tensors(64)      # float32 [64,15,10,9], [64,1] on the GPU
    states, targets, pt = buf.sample_policy_tensors(64)   # ... plus PolicyTarget(cols, pi, n_moves) on the GPU
    boards, move_probs_list, rewards = buf.sample(64)   # the reference's return value

`sample*` draws its indices exactly like the reference: np.random.choice(len, batch, replace=False)
on NumPy's global stream (trainer.py:37).  `sample` hands back the very tuples `push` was given
(trainer.py:27-42 keeps the tuples themselves): a host-side table beside the device ring remembers
them per ring position, so pushed probabilities come back exactly; records that arrived from the
device (`push_records`) are decoded from their visit counts.  States are encode_board(board, 1) — the player plane is
hard-wired to red in the reference's trainer (trainer.py:314).  `sample_tensors` hands out z alone, what the
reference's value-only loss uses (trainer.py:324-331); `sample_policy_tensors` adds the policy target that loss
leaves out ("完整版需要把move_probs转换为target policy"): pi over each record's moves and their policy columns, formed
on the device from the ring (training.policy_loss consumes it).  That target comes from the record's visit counts,
for pushed tuples too: `push` stores round(p * 65535) as counts, so a pushed distribution comes back at 16-bit
resolution there (exactly from `sample`).
"""
import collections
import ctypes as C

import numpy as np

from . import _lib
from .chess_env import decode_move, encode_move
from .distributed import RECORD_BYTES, RECORD_DTYPE, record_to_sample

# the policy target of a batch, all on the device: cols int32 [B,128] (policy column of every move, -1 = none),
# pi float32 [B,128] (0 from n_moves on), n_moves int32 [B]
PolicyTarget = collections.namedtuple("PolicyTarget", ["cols", "pi", "n_moves"])
MAX_COUNT = 65535                                  # the record's counts are uint16


def pack_board_words(board):
    b = np.asarray(board, dtype=np.int16).reshape(90)
    code = np.where(b > 0, b, np.where(b < 0, 7 - b, 0)).astype(np.uint32)
    w = np.zeros(12, np.uint32)
    for s in range(90):
        w[s // 8] |= code[s] << np.uint32(4 * (s % 8))
    return w


class ReplayBuffer:
    def __init__(self, max_size=10000, device=0, temperature=1.0):
        self.L = _lib.lib()
        h = C.c_void_p()
        rc = self.L.xq_replay_create(device, max_size, C.byref(h))
        if rc != 0:
            raise _lib.XqError("xq_replay_create failed (%d): %s — the replay buffer is device-resident, "
                               "there is no CPU fallback" % (rc, self.L.xq_replay_last_error().decode()))
        self.h = h
        self.max_size = max_size
        self.temperature = temperature
        # one entry per ring position, oldest first, in step with the device ring (same maxlen, same append order):
        # the tuple `push` was given, or None for a record that came from the device
        self._host = collections.deque(maxlen=max_size)
        self._pow_tables = {}                      # temperature -> device float64[65536]: counts ** (1/T) as numpy evaluates it
        self._column_maps = {}                     # id(host map) -> (host map, device int32[8100])

    def _chk(self, rc):
        if rc != 0:
            raise _lib.XqError("libxq_hip replay error %d: %s" % (rc, self.L.xq_replay_last_error().decode()))

    def close(self):
        if getattr(self, "h", None):
            self.L.xq_replay_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __len__(self):
        return int(self.L.xq_replay_size(self.h))

    @staticmethod
    def _stream():
        import torch
        return torch.cuda.current_stream().cuda_stream

    def push_records(self, records, n_games):
        """records: uint8 CUDA tensor holding xq_sample_record[n_games][70] (engine.pack_samples or
        distributed.all_gather_records output).  Appends every valid record, oldest dropped first."""
        assert records.is_cuda and records.numel() >= n_games * _lib.MAX_PLIES * RECORD_BYTES
        n = C.c_int64()
        self._chk(self.L.xq_replay_push_records(self.h, C.c_void_p(self._stream()), C.c_void_p(records.data_ptr()),
                                                 int(n_games), C.byref(n)))
        self._host.extend([None] * min(n.value, self.max_size))
        return n.value

    def push(self, game_data):
        """trainer.py:27-33 for one game in the reference's tuple format [(board, {move: prob}, z)].  Boards and z
        go to the device ring (they are what batch formation reads, trainer.py:313-321); the tuples themselves are
        kept host-side and returned by sample() unchanged, as the reference's deque does.  Nothing is truncated: a
        game longer than 70 samples spans several 70-record blocks; a sample with more than 128 moves does not fit
        the record and raises."""
        import torch
        game_data = list(game_data)
        if not game_data:
            return 0
        nblk = (len(game_data) + _lib.MAX_PLIES - 1) // _lib.MAX_PLIES
        rec = np.zeros((nblk, _lib.MAX_PLIES), dtype=RECORD_DTYPE)
        for i, (board, move_probs, z) in enumerate(game_data):
            r = rec[i // _lib.MAX_PLIES, i % _lib.MAX_PLIES]
            moves = list(move_probs.keys())
            if len(moves) > _lib.MAX_MOVES:
                raise ValueError("ReplayBuffer.push: sample %d has %d moves; a sample record holds %d"
                                 % (i, len(moves), _lib.MAX_MOVES))
            r["board"] = pack_board_words(board)
            r["z"] = float(z)
            r["player"] = 0
            r["n_moves"] = len(moves)
            r["valid"] = 1
            r["moves"][:len(moves)] = [encode_move(m) for m in moves]
            # (the record's 16-bit counts cannot hold probabilities: they stay a coarse view for tools that read raw
            # records; sample() returns the pushed tuple itself)
            r["counts"][:len(moves)] = [int(round(min(max(float(move_probs[m]), 0.0), 1.0) * 65535)) for m in moves]
        t = torch.from_numpy(np.frombuffer(rec.tobytes(), dtype=np.uint8).copy()).cuda()
        n = C.c_int64()
        self._chk(self.L.xq_replay_push_records(self.h, C.c_void_p(self._stream()), C.c_void_p(t.data_ptr()),
                                                 int(nblk), C.byref(n)))
        assert n.value == len(game_data)
        self._host.extend(game_data)
        return n.value

    def _indices(self, batch_size):
        return np.ascontiguousarray(np.random.choice(len(self), batch_size, replace=False), dtype=np.int64)   # trainer.py:37

    def sample_tensors(self, batch_size, indices=None):
        """Device-side batch formation: (states float32 [B,15,10,9], targets float32 [B,1])."""
        import torch
        idx = self._indices(batch_size) if indices is None else np.ascontiguousarray(indices, dtype=np.int64)
        states = torch.empty((len(idx), 15, 10, 9), dtype=torch.float32, device="cuda")
        targets = torch.empty((len(idx), 1), dtype=torch.float32, device="cuda")
        self._chk(self.L.xq_replay_encode_batch(self.h, C.c_void_p(self._stream()), _lib.ptr(idx), len(idx),
                                                 C.c_void_p(states.data_ptr()), C.c_void_p(targets.data_ptr())))
        return states, targets

    def _pow_table(self, temperature):
        """counts ** (1/T) for every uint16 count exactly as record_to_sample's numpy evaluates it (the engine does the
        same for its sampler, xq_engine_set_pow_table); T = 1 and the argmax branch need none"""
        import torch
        if temperature < 0.01 or temperature == 1.0:
            return None
        if temperature not in self._pow_tables:
            tab = np.ascontiguousarray(np.arange(MAX_COUNT + 1, dtype=np.int64) ** (1.0 / temperature), dtype=np.float64)
            self._pow_tables[temperature] = torch.from_numpy(tab).cuda()
        return self._pow_tables[temperature]

    def _column_map(self, column_map):
        """move -> policy column as a device int32[8100]; host tables (InferenceNet.column_map, the second value of
        reachable_policy_columns()) are uploaded once per table"""
        import torch
        if column_map is None:
            return None
        if torch.is_tensor(column_map):
            if not (column_map.is_cuda and column_map.dtype == torch.int32 and column_map.is_contiguous()
                    and column_map.numel() == _lib.POLICY_SIZE):
                raise ValueError("column_map tensor must be a contiguous int32 CUDA tensor of %d entries" % _lib.POLICY_SIZE)
            return column_map
        key = id(column_map)
        if key not in self._column_maps or self._column_maps[key][0] is not column_map:
            host = np.asarray(column_map)
            if host.shape != (_lib.POLICY_SIZE,):
                raise ValueError("column_map must have %d entries" % _lib.POLICY_SIZE)
            self._column_maps[key] = (column_map, torch.from_numpy(np.ascontiguousarray(host, dtype=np.int32)).cuda())
        return self._column_maps[key][1]

    def sample_policy_tensors(self, batch_size, indices=None, temperature=None, column_map=None, mirror=None,
                              player_plane="red"):
        """Device-side batch formation with the policy target: (states float32 [B,15,10,9], target_values float32 [B,1],
        PolicyTarget(cols int32 [B,128], pi float32 [B,128], n_moves int32 [B])), everything on the GPU.
        pi[b, i] = float32(counts[i] ** (1/T) / sum), the float64 arithmetic of record_to_sample(rec, T) rounded once
        (T < 0.01: 1 on the first maximum); `temperature` defaults to the buffer's.  cols[b, i] = the policy column of
        moves[i]: from*90+to (neural_network.py:160), or column_map[from*90+to] with a `column_map` (int[8100], -1 =
        no column: InferenceNet.column_map / reachable_policy_columns()[1], or a device int32 tensor); -1 from n_moves on.
        `mirror`: None, or a bool / 0-1 array [B]: those samples are flipped left-right (board files and the moves'
        squares; pi unchanged) - a legal sample by the symmetry of the rules, off by default as in the reference.
        `player_plane`: "red" = plane 14 all ones, the reference trainer's hard-wired encode_board(board, 1)
        (trainer.py:314); "record" = the side to move stored with the record (encode_board(board, player)).  Records
        that came through push() carry no side (player 0): their plane is 0 in that mode.
        Without `indices` they are drawn exactly as sample_tensors draws them (trainer.py:37)."""
        import torch
        if player_plane not in ("red", "record"):
            raise ValueError("player_plane must be 'red' or 'record'")
        idx = self._indices(batch_size) if indices is None else np.ascontiguousarray(indices, dtype=np.int64)
        B = len(idx)
        T = float(self.temperature if temperature is None else temperature)
        flags = None
        if mirror is not None:
            flags = np.ascontiguousarray(np.broadcast_to(np.asarray(mirror), (B,)) != 0, dtype=np.uint8)
        tab = self._pow_table(T)
        cmap = self._column_map(column_map)
        states = torch.empty((B, 15, 10, 9), dtype=torch.float32, device="cuda")
        targets = torch.empty((B, 1), dtype=torch.float32, device="cuda")
        cols = torch.empty((B, _lib.MAX_MOVES), dtype=torch.int32, device="cuda")
        pi = torch.empty((B, _lib.MAX_MOVES), dtype=torch.float32, device="cuda")
        n_moves = torch.empty((B,), dtype=torch.int32, device="cuda")
        self._chk(self.L.xq_replay_encode_policy_batch(
            self.h, C.c_void_p(self._stream()), _lib.ptr(idx), B, _lib.ptr(flags), 1 if player_plane == "record" else 0, T,
            C.c_void_p(tab.data_ptr()) if tab is not None else None, tab.numel() if tab is not None else 0,
            C.c_void_p(cmap.data_ptr()) if cmap is not None else None,
            C.c_void_p(states.data_ptr()), C.c_void_p(targets.data_ptr()), C.c_void_p(cols.data_ptr()),
            C.c_void_p(pi.data_ptr()), C.c_void_p(n_moves.data_ptr())))
        return states, targets, PolicyTarget(cols, pi, n_moves)

    def sample(self, batch_size, indices=None):
        """trainer.py:35-42: (boards, move_probs_list, rewards) tuples of length batch_size."""
        idx = self._indices(batch_size) if indices is None else np.ascontiguousarray(indices, dtype=np.int64)
        assert len(self._host) == len(self)
        rec = np.zeros(len(idx), dtype=RECORD_DTYPE)
        self._chk(self.L.xq_replay_read_records(self.h, C.c_void_p(self._stream()), _lib.ptr(idx), len(idx), _lib.ptr(rec)))
        out = [self._host[int(i)] if self._host[int(i)] is not None else record_to_sample(r, self.temperature)
               for i, r in zip(idx, rec)]
        boards, probs, rewards = zip(*out)
        return boards, probs, rewards
