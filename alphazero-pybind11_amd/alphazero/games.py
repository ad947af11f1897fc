"""The game-state classes of the five device games: byte layouts, pickling, __str__ dumps, and the batched rules /
symmetry entry points."""
import ctypes as C
import struct

import numpy as np

from ._capi import lib, check
from .params import PlayHistory


def symmetries_batch(game_cls, canonical, v, pi, device=0, stream=None):
    """All NUM_SYMMETRIES images of a batch of samples in one launch (azmi_symmetries).
    numpy in -> numpy out ([n, NS, ...]); torch CUDA tensors in -> torch CUDA tensors out, no host copy."""
    ns = game_cls.NUM_SYMMETRIES()
    P, M, chw = game_cls._info()
    if hasattr(canonical, "is_cuda"):
        import torch
        if not (canonical.is_cuda and v.is_cuda and pi.is_cuda):
            raise RuntimeError("symmetries_batch: torch inputs must be CUDA tensors (numpy arrays take the staged path)")
        c = canonical.contiguous().float(); vv = v.contiguous().float(); pp = pi.contiguous().float()
        n = c.shape[0]
        if tuple(c.shape[1:]) != tuple(chw) or tuple(vv.shape) != (n, P + 1) or tuple(pp.shape) != (n, M):
            raise RuntimeError("Improper sample shapes")
        oc = torch.empty((n, ns) + tuple(chw), dtype=torch.float32, device=c.device)
        ov = torch.empty((n, ns, P + 1), dtype=torch.float32, device=c.device)
        op = torch.empty((n, ns, M), dtype=torch.float32, device=c.device)
        st = torch.cuda.current_stream(c.device).cuda_stream if stream is None else stream
        rc = lib.azmi_symmetries(game_cls.GAME_ID, c.device.index, n, c.data_ptr(), vv.data_ptr(), pp.data_ptr(),
                                 oc.data_ptr(), ov.data_ptr(), op.data_ptr(), 0, C.c_void_p(st))
        if rc:
            raise RuntimeError(lib.azmi_symmetries_last_error().decode())
        return oc, ov, op
    c = np.ascontiguousarray(canonical, np.float32); vv = np.ascontiguousarray(v, np.float32)
    pp = np.ascontiguousarray(pi, np.float32)
    n = c.shape[0]
    if tuple(c.shape[1:]) != tuple(chw) or vv.shape != (n, P + 1) or pp.shape != (n, M):
        raise RuntimeError("Improper sample shapes")
    oc = np.zeros((n, ns) + tuple(chw), np.float32); ov = np.zeros((n, ns, P + 1), np.float32)
    op = np.zeros((n, ns, M), np.float32)
    rc = lib.azmi_symmetries(game_cls.GAME_ID, device, n, c.ctypes.data, vv.ctypes.data, pp.ctypes.data,
                             oc.ctypes.data, ov.ctypes.data, op.ctypes.data, 1, None)
    if rc:
        raise RuntimeError(lib.azmi_symmetries_last_error().decode())
    return oc, ov, op


def tafl_symmetries(board, canonical, v, pi, device=0):
    """eightSym for any square Tafl board (azmi_tafl_symmetries), numpy [n,...] in/out."""
    c = np.ascontiguousarray(canonical, np.float32); vv = np.ascontiguousarray(v, np.float32)
    pp = np.ascontiguousarray(pi, np.float32)
    n, ch = c.shape[0], c.shape[1]
    oc = np.zeros((n, 8) + c.shape[1:], np.float32); ov = np.zeros((n, 8, vv.shape[1]), np.float32)
    op = np.zeros((n, 8, pp.shape[1]), np.float32)
    if c.shape[2:] != (board, board) or pp.shape[1] != board * board * 2 * board:
        raise RuntimeError("Improper sample shapes")
    rc = lib.azmi_tafl_symmetries(board, ch, vv.shape[1], device, n, c.ctypes.data, vv.ctypes.data, pp.ctypes.data,
                                  oc.ctypes.data, ov.ctypes.data, op.ctypes.data, 1, None)
    if rc:
        raise RuntimeError(lib.azmi_symmetries_last_error().decode())
    return oc, ov, op


class GameState:
    """A game position (py_wrapper.cc:157-189).  The object is a start position plus the moves played
    from it; every query (valid_moves, scores, canonicalized, ...) is answered by the device rules
    kernels (azmi_game_replay_from) and memoised until the next play_move()."""

    GAME_ID = -1
    _REPLAY_FLAGS = 0          # bit 0: reference-style unchecked play_move (Brandubh / OpenTafl objects)

    def __init__(self):
        self._init = None      # serialized start position (reference pickle image) or None = initial()
        self._moves = []
        self._snap = None
        self._device = 0

    # ---- statics ---------------------------------------------------------------------------
    @classmethod
    def _info(cls):
        p, m = C.c_uint32(), C.c_uint32()
        chw = (C.c_uint32 * 3)()
        check(lib.azmi_game_info(cls.GAME_ID, C.byref(p), C.byref(m), chw))
        return p.value, m.value, tuple(chw)

    @classmethod
    def NUM_PLAYERS(cls):
        return cls._info()[0]

    @classmethod
    def NUM_MOVES(cls):
        return cls._info()[1]

    @classmethod
    def CANONICAL_SHAPE(cls):
        return cls._info()[2]

    # ---- instance surface ------------------------------------------------------------------
    def _state(self):
        if self._snap is None:
            P, M, chw = self._info()
            mv = np.array([self._moves + [-1]], dtype=np.int32)
            out = dict(valid=np.zeros((1, M), np.uint8), scores=np.zeros((1, P + 1), np.float32),
                       canonical=np.zeros((1,) + tuple(chw), np.float32), player=np.zeros(1, np.uint32),
                       turn=np.zeros(1, np.uint32), key=np.zeros(1, np.uint64), status=np.zeros(1, np.int32))
            init = None if self._init is None else np.frombuffer(self._init, np.uint8)
            check(lib.azmi_game_replay_ex(self.GAME_ID, self._device, None if init is None else init.ctypes.data,
                                          0 if init is None else init.size, mv.ctypes.data, 1, mv.shape[1],
                                          out["valid"].ctypes.data, out["scores"].ctypes.data, out["canonical"].ctypes.data,
                                          out["player"].ctypes.data, out["turn"].ctypes.data, out["key"].ctypes.data,
                                          out["status"].ctypes.data, self._REPLAY_FLAGS))
            if out["status"][0] != 0:
                raise RuntimeError("illegal move in the game record")
            self._snap = out
        return self._snap

    def copy(self):
        g = self.__class__.__new__(self.__class__)
        g.__dict__.update(self.__dict__)
        g._moves = list(self._moves)
        return g

    def __eq__(self, other):
        if not isinstance(other, GameState) or other.GAME_ID != self.GAME_ID:
            return False
        a, b = self._state(), other._state()
        return bool(a["player"][0] == b["player"][0] and a["turn"][0] == b["turn"][0]
                    and np.array_equal(a["canonical"], b["canonical"]))

    __hash__ = None

    def current_turn(self):
        return int(self._state()["turn"][0])

    def current_player(self):
        return int(self._state()["player"][0])

    def num_players(self):
        return self.NUM_PLAYERS()

    def num_moves(self):
        return self.NUM_MOVES()

    def num_symmetries(self):
        return self.NUM_SYMMETRIES()

    def relative_values(self):   # game_state.h:114
        return False

    def randomize_start(self):   # game_state.h:73 — a no-op except for StarGambitUnifiedGS (which re-draws its variant)
        return None

    def num_variants(self):      # game_state.h:76
        return 0

    def get_variant_id(self):    # game_state.h:79
        return -1

    def valid_moves(self):
        return self._state()["valid"][0].copy()

    def play_move(self, move):
        move = int(move)
        if not 0 <= move < self.NUM_MOVES():
            raise RuntimeError(f"move {move} out of range")
        self._moves.append(move)
        self._snap = None

    def scores(self):
        sc = self._state()["scores"][0]
        return None if sc[0] < 0 else sc.copy()

    def canonicalized(self):
        return self._state()["canonical"][0].copy()

    def symmetries(self, base):
        """GameState::symmetries(PlayHistory) -> list of NUM_SYMMETRIES PlayHistory (device gather)."""
        oc, ov, op = symmetries_batch(self.__class__, base._c[None], base._v[None], base._pi[None], device=self._device)
        return [PlayHistory(oc[0, i], ov[0, i], op[0, i]) for i in range(oc.shape[1])]


class Connect4GS(GameState):  # py_wrapper.cc:562-586
    GAME_ID = 0
    MAX_TURNS = 42             # board cells

    def __init__(self, board=None, player=0, turn=0):
        super().__init__()
        if board is not None:
            b = np.ascontiguousarray(board, dtype=np.int8)
            if b.shape != (2, 6, 7):
                raise RuntimeError("Improper connect 4 board shape")
            self._init = b.tobytes() + np.int8(player).tobytes() + np.int32(turn).tobytes()

    @staticmethod
    def NUM_SYMMETRIES():
        return 2

    def play_move(self, move):
        """connect4_gs.cc:48-58: a move into a full column throws at once (the object stays as it was)."""
        super().play_move(move)
        try:
            self._state()
        except RuntimeError:
            self._moves.pop()
            self._snap = None
            raise RuntimeError("Invalid move: You have a bug in your code.") from None

    def to_bytes(self):          # connect4_gs.cc:172-178
        st = self._state()
        board = (st["canonical"][0, :2] != 0).astype(np.int8)
        return board.tobytes() + np.int8(st["player"][0]).tobytes() + np.int32(st["turn"][0]).tobytes()

    @classmethod
    def from_bytes(cls, data):   # connect4_gs.cc:180-190
        if len(data) != 89:
            raise ValueError("Connect4GS::from_bytes: wrong size")
        g = cls()
        g._init = bytes(data)
        return g

    def __reduce__(self):        # ADD_GS_PICKLE, py_wrapper.cc:77-83
        return (_c4_from_bytes, (self.to_bytes(),))

    def __str__(self):           # connect4_gs.cc:192-208
        st = self._state()
        out = "Current Player: %d\n" % st["player"][0]
        for h in range(6):
            out += "".join("X" if st["canonical"][0, 0, h, w] == 1 else "O" if st["canonical"][0, 1, h, w] == 1 else "."
                           for w in range(7)) + "\n"
        return out + "\n"


def _c4_from_bytes(data):
    return Connect4GS.from_bytes(data)


class _TaflBoardGS(GameState):
    """Tafl-family objects.  A start position other than the game's own is the REFERENCE's pickle image
    (tawlbwrdd_gs.cc:10-37, brandubh_gs.cc:11-41, opentafl_gs.cc:13-40):
        board int8[3][N][N] (king, defenders, attackers) | u16 turn | u16 max_turns | i8 player | u8 current_repetition_count |
        u32 n | n x (board | u8 player | u8 count)                       (little endian)
    so a state pickled by the reference loads here and the other way round, repetition map included."""
    BOARD = 0
    MAX_TURNS = 0
    _REPLAY_FLAGS = 1          # play_move like the reference: no ownership / slide check (valid_moves is the validator)

    def __init__(self, max_turns=None):
        super().__init__()
        if max_turns is not None and max_turns != self.MAX_TURNS:
            raise RuntimeError(f"the MI355X engine implements {type(self).__name__} with the default max_turns = {self.MAX_TURNS}")

    @classmethod
    def _image(cls, board, player, turn, rep_count=1, entries=()):
        b = np.ascontiguousarray(board, dtype=np.int8)
        if b.shape != (3, cls.BOARD, cls.BOARD):
            raise RuntimeError("Improper tafl board shape")
        out = [b.tobytes(), np.uint16(turn).tobytes(), np.uint16(cls.MAX_TURNS).tobytes(), np.int8(player).tobytes(),
               np.uint8(rep_count).tobytes(), np.uint32(len(entries)).tobytes()]
        for eb, ep, ec in entries:
            out += [eb, np.uint8(ep).tobytes(), np.uint8(ec).tobytes()]
        return b"".join(out)

    @classmethod
    def from_board(cls, board, player, turn=0):
        """the C++ test helper MakeGS (opentafl_gs_test.cc:97-101): a board with an empty repetition map, count 1"""
        g = cls()
        g._init = cls._image(board, player, turn)
        return g

    @classmethod
    def from_bytes(cls, data):
        data = bytes(data)
        bb = 3 * cls.BOARD * cls.BOARD
        if len(data) < bb + 10:
            raise RuntimeError(f"{cls.__name__}::from_bytes: data too short")
        n = int(np.frombuffer(data[bb + 6: bb + 10], np.uint32)[0])
        if bb + 10 + n * (bb + 2) != len(data):
            raise RuntimeError(f"{cls.__name__}::from_bytes: repetition entry count mismatch")
        if int(np.frombuffer(data[bb + 2: bb + 4], np.uint16)[0]) != cls.MAX_TURNS:
            raise RuntimeError(f"the MI355X engine implements {cls.__name__} with the default max_turns = {cls.MAX_TURNS}")
        g = cls()
        g._init = data
        return g

    def to_bytes(self):
        """The reference's to_bytes image of the current position.  The repetition map holds boards, the device keeps
        64-bit keys, so the boards are read back by replaying every prefix of the game record (one batched device call)
        and applying the reference's bookkeeping: the start position is interned by the first move of a game, a capture
        clears the map, every move counts the position it reaches (tawlbwrdd_gs.cc:253-259, 286-331)."""
        if not self._moves and self._init is not None:
            return self._init
        P, M, chw = self._info()
        L = len(self._moves)
        mv = np.full((L + 1, L + 1), -1, np.int32)
        for i in range(L + 1):
            mv[i, :i] = self._moves[:i]
        canon = np.zeros((L + 1,) + tuple(chw), np.float32)
        player = np.zeros(L + 1, np.uint32); turn = np.zeros(L + 1, np.uint32); status = np.zeros(L + 1, np.int32)
        init = None if self._init is None else np.frombuffer(self._init * (L + 1), np.uint8)
        check(lib.azmi_game_replay_ex(self.GAME_ID, self._device, None if init is None else init.ctypes.data,
                                      0 if init is None else len(self._init), mv.ctypes.data, L + 1, L + 1,
                                      None, None, canon.ctypes.data, player.ctypes.data, turn.ctypes.data, None, status.ctypes.data,
                                      self._REPLAY_FLAGS))
        if status.any():
            raise RuntimeError("illegal move in the game record")
        boards = (canon[:, :3] != 0).astype(np.int8)
        pieces = boards.reshape(L + 1, -1).sum(1)
        bb = 3 * self.BOARD * self.BOARD
        reps = []                                   # (board bytes, player) in insertion order, with multiplicity
        rep_count = 1
        if self._init is not None:
            rep_count = self._init[bb + 5]
            n = int(np.frombuffer(self._init[bb + 6: bb + 10], np.uint32)[0])
            for e in range(n):
                o = bb + 10 + e * (bb + 2)
                reps += [(self._init[o: o + bb], self._init[o + bb])] * self._init[o + bb + 1]
        for i in range(1, L + 1):
            if turn[i - 1] == 0:
                reps = [(boards[i - 1].tobytes(), int(player[i - 1]))]
            if pieces[i] < pieces[i - 1]:
                reps = []
            key = (boards[i].tobytes(), int(player[i]))
            reps.append(key)
            rep_count = reps.count(key)
        entries, seen = [], {}
        for key in reps:
            if key in seen:
                entries[seen[key]][2] += 1
            else:
                seen[key] = len(entries)
                entries.append([key[0], key[1], 1])
        return self._image(boards[L], int(player[L]), int(turn[L]), rep_count, entries)

    def __reduce__(self):        # ADD_GS_PICKLE, py_wrapper.cc:77-83
        return (_tafl_from_bytes, (type(self).__name__, self.to_bytes()))

    @staticmethod
    def NUM_SYMMETRIES():
        return 8

    @classmethod
    def POLICY_SHAPE(cls):
        return (2 * cls.BOARD, cls.BOARD, cls.BOARD)

    def _rep_count(self):
        st = self._state()
        c = st["canonical"][0]
        return 3 if (c[5, 0, 0] and c[6, 0, 0] and st["turn"][0] > 0) else 2 if c[6, 0, 0] else 1 if c[5, 0, 0] else 0

    def __str__(self):           # brandubh_gs.cc:547-581 / opentafl_gs.cc:589-623 without the colour escapes
        st = self._state()
        c = st["canonical"][0]
        out = "Current Player: %d\nCurrent Turn: %d out of %d\n" % (st["player"][0], st["turn"][0], self.MAX_TURNS)
        for h in range(self.BOARD):
            out += "".join("@" if c[0, h, w] == 1 else "O" if c[1, h, w] == 1 else "X" if c[2, h, w] == 1 else "."
                           for w in range(self.BOARD)) + "\n"
        return out + "\n"


def _tafl_from_bytes(name, data):
    return {"TawlbwrddGS": TawlbwrddGS, "BrandubhGS": BrandubhGS, "OpenTaflGS": OpenTaflGS}[name].from_bytes(data)


class TawlbwrddGS(_TaflBoardGS):  # py_wrapper.cc:549-560
    GAME_ID = 1
    BOARD = 11
    MAX_TURNS = 400
    _REPLAY_FLAGS = 0

    def __str__(self):           # tawlbwrdd_gs.cc:460-484
        st = self._state()
        c = st["canonical"][0]
        out = "Current Player: %d\nCurrent Turn: %d out of 400\nCurrent Repetition Count: %d\n" % (st["player"][0], st["turn"][0], self._rep_count())
        for h in range(11):
            out += "".join("@" if c[0, h, w] == 1 else "O" if c[1, h, w] == 1 else "X" if c[2, h, w] == 1 else "."
                           for w in range(11)) + "\n"
        return out + "\n"


class BrandubhGS(_TaflBoardGS):  # py_wrapper.cc:527-536
    GAME_ID = 2
    BOARD = 7
    MAX_TURNS = 150


class OpenTaflGS(_TaflBoardGS):  # py_wrapper.cc:538-547
    GAME_ID = 3
    BOARD = 11
    MAX_TURNS = 400


class UnitInfo:
    """UnitInfo of get_units() (star_gambit_gs.h:424-433, py_wrapper.cc StarGambit bindings)."""
    __slots__ = ("player", "type", "slot", "hp", "anchor_q", "anchor_r", "facing", "moves_left")

    def __init__(self, player, type, slot, hp, anchor_q, anchor_r, facing, moves_left):
        self.player, self.type, self.slot, self.hp = player, type, slot, hp
        self.anchor_q, self.anchor_r, self.facing, self.moves_left = anchor_q, anchor_r, facing, moves_left

    def __repr__(self):
        return (f"UnitInfo(player={self.player}, type={self.type}, slot={self.slot}, hp={self.hp}, "
                f"anchor=({self.anchor_q}, {self.anchor_r}), facing={self.facing}, moves_left={self.moves_left})")


class StarGambitUnifiedGS(GameState):
    """StarGambitUnifiedGS(pinned_variant=-1, probs=[.25]*4) (py_wrapper.cc:662-667; star_gambit_gs.h:788-887): the four
    configurations on the 13 x 13 canvas.  The object is the reference's to_bytes image of a start position plus the moves
    played from it; the device rules (csrc/dev_stargambit.h, one wavefront per object) answer every query.

    Build-defined: the reference draws the variant of an unpinned game from an unseedable thread-local engine
    (star_gambit_gs.cc:2357-2362); here the constructor / randomize_start() draw it from Python's `random` module, and a
    PlayManager draws every game's variant from the slot's coin stream."""

    GAME_ID = 4
    MAX_TURNS = 4096           # the engine's bound on the ACTIONS of a game (csrc/dev_stargambit.h)
    _REPLAY_FLAGS = 1          # play_move does not validate, like the reference's (star_gambit_gs.cc:1093-1238)
    _VARIANT_NAMES = ("Skirmish", "Showdown", "Clash", "Battle")

    def __init__(self, pinned_variant=-1, probs=(0.25, 0.25, 0.25, 0.25)):
        super().__init__()
        self._pinned = int(pinned_variant)
        self._probs = tuple(float(x) for x in probs)
        if len(self._probs) != 4:
            raise TypeError("probs must have four entries")
        self._start_variant(self._pick_variant())

    def _pick_variant(self):
        if 0 <= self._pinned <= 3:
            return self._pinned
        import random
        return random.choices(range(4), weights=self._probs)[0]

    def _start_variant(self, v):
        """the start position of variant v: two portals, full reserves, the position seen once (star_gambit_gs.cc:251-290)"""
        side = 6 if v == 3 else 5
        start = ((3, 1, 0), (4, 0, 1), (3, 2, 1), (4, 3, 2))[v]
        units = bytes([3, 0, 0, 5, 2, 0, side, 0, 0]) + bytes([3, 1, 0, 5, 5, 0, (-side) & 0xFF, 0, 0])

        def uh(t, pl, hp, f, q, r):
            return ((t ^ (pl << 8) ^ (hp << 12) ^ (f << 20) ^ ((q + 10) << 28) ^ ((r + 10) << 36)) * 0x517cc1b727220a95) & (2**64 - 1)
        h0 = uh(3, 0, 5, 2, 0, side) ^ uh(3, 1, 5, 5, 0, -side)     # compute_position_hash with player 0 to move, :1365-1382
        inner = (struct.pack("<I", 2) + units + bytes(start) + b"\0" + bytes(start) + b"\0" + struct.pack("<BIBBbI", 0, 1, 0, 0, -1, 1)
                 + struct.pack("<Q", h0))
        self._init = self._header(v, len(inner)) + inner
        self._moves = []
        self._snap = None
        self._img = None

    def _header(self, variant, inner_size):
        return struct.pack("<4fiBI", *self._probs, self._pinned, variant, inner_size)

    @staticmethod
    def NUM_SYMMETRIES():
        return 2

    @classmethod
    def POLICY_SHAPE(cls):         # star_gambit_gs.h:818-819; neural_net.py:281 keys the spatial policy head on it
        return (10, 13, 13)

    def relative_values(self): return True           # star_gambit_gs.h:845
    def num_variants(self): return 4                 # :863
    def get_variant_id(self): return self._image()[20]

    def randomize_start(self):                       # star_gambit_gs.cc:2421-2425
        self._start_variant(self._pick_variant())

    def _image(self):
        """to_bytes image of the current position (device: azmi_sg_image); cached per move count (MCTS.find_leaf appends moves)"""
        cached = getattr(self, "_img", None)
        if cached is not None and cached[0] == len(self._moves):
            return cached[1]
        self._img = (len(self._moves), self._make_image())
        return self._img[1]

    def _make_image(self):
        if True:
            if not self._moves:
                return bytes(self._init)
            else:
                mv = np.array([self._moves + [-1]], dtype=np.int32)
                init = np.frombuffer(self._init, np.uint8)
                cap = len(self._init) + 9 * 20 + 8 * (len(self._moves) + 4) + 64
                out = np.zeros(cap, np.uint8); n = np.zeros(1, np.uint32); st = np.zeros(1, np.int32)
                check(lib.azmi_sg_image(self._device, init.ctypes.data, init.size, mv.ctypes.data, 1, mv.shape[1], out.ctypes.data, cap,
                                        n.ctypes.data, st.ctypes.data, self._REPLAY_FLAGS))
                if st[0] != 0:
                    raise RuntimeError("illegal move in the game record")
                b = bytearray(out[: int(n[0])].tobytes())
                b[:20] = struct.pack("<4fi", *self._probs, self._pinned)
                return bytes(b)

    def to_bytes(self):                              # star_gambit_gs.cc:2451-2465
        return self._image()

    @classmethod
    def from_bytes(cls, data):                       # star_gambit_gs.cc:2467-2516
        data = bytes(data)
        if len(data) < 25:
            raise RuntimeError("StarGambitUnifiedGS::from_bytes: short data")
        probs = struct.unpack_from("<4f", data, 0)
        pinned, variant, inner_size = struct.unpack_from("<iBI", data, 16)
        if variant > 3:
            raise RuntimeError("StarGambitUnifiedGS::from_bytes: bad variant_id")
        if 25 + inner_size > len(data):
            raise RuntimeError("StarGambitUnifiedGS::from_bytes: short inner")
        if 25 + inner_size != len(data):
            raise RuntimeError("StarGambitUnifiedGS::from_bytes: trailing bytes")
        g = cls.__new__(cls)
        GameState.__init__(g)
        g._pinned, g._probs = int(pinned), tuple(float(x) for x in probs)
        g._init, g._moves, g._snap, g._img = data, [], None, None
        g._state()        # the device parses the inner image: malformed images raise here
        return g

    def __reduce__(self):                            # ADD_GS_PICKLE, py_wrapper.cc:77-83
        return (_sg_from_bytes, (type(self).__name__, self.to_bytes()))

    def _fields(self):
        b = self._image()
        n = struct.unpack_from("<I", b, 25)[0]
        units = [struct.unpack_from("<5B2b2B", b, 29 + 9 * i) for i in range(n)]
        off = 29 + 9 * n
        reserves = list(b[off:off + 8])
        player, turn, acted, over, winner, hist = struct.unpack_from("<BIBBbI", b, off + 8)
        return units, reserves, player, turn, bool(acted), bool(over), winner, hist

    def get_units(self):                             # alive units only, star_gambit_gs.cc:2102-2118
        return [UnitInfo(u[1], u[0], u[2], u[3], u[5], u[6], u[4], u[7]) for u in self._fields()[0] if u[3] > 0]

    def has_taken_action(self):                      # star_gambit_gs.h:654
        return self._fields()[4]

    def __eq__(self, other):                         # operator==, star_gambit_gs.cc:297-319, 2392-2397: turn and history take no part
        if not isinstance(other, StarGambitUnifiedGS):
            return False
        a, b = self._fields(), other._fields()
        return self.get_variant_id() == other.get_variant_id() and a[0] == b[0] and a[1] == b[1] and a[2] == b[2] and a[4] == b[4]

    __hash__ = None

    def dump(self):                                  # star_gambit_gs.cc:1807-1830 (header lines)
        units, res, player, turn, acted, over, winner, _ = self._fields()
        return (f"Turn: {turn}, Player: {player}{' (acted)' if acted else ''}\n"
                f"P0 reserves: F={res[0]} C={res[1]} D={res[2]}\nP1 reserves: F={res[4]} C={res[5]} D={res[6]}\n"
                + "".join(f"P{u[1]} {'FCDP'[u[0]]}{u[2] + 1} hp={u[3]} at ({u[5]}, {u[6]}) facing {u[4]}\n" for u in units if u[3] > 0))

    __str__ = dump

    # symmetries(PlayHistory): GameState.symmetries -> azmi_symmetries(AZMI_GAME_STARGAMBIT): {base, NW-axis mirror},
    # star_gambit_gs.cc:2623-2727


def _pinned_sg(name, variant):
    def __init__(self):
        StarGambitUnifiedGS.__init__(self, variant)
    return type(name, (StarGambitUnifiedGS,), {"__init__": __init__, "__doc__": f"StarGambitUnifiedGS pinned to {name[17:-2]} (star_gambit_gs.h:893-911)"})


StarGambitUnifiedSkirmishGS = _pinned_sg("StarGambitUnifiedSkirmishGS", 0)
StarGambitUnifiedShowdownGS = _pinned_sg("StarGambitUnifiedShowdownGS", 1)
StarGambitUnifiedClashGS = _pinned_sg("StarGambitUnifiedClashGS", 2)
StarGambitUnifiedBattleGS = _pinned_sg("StarGambitUnifiedBattleGS", 3)


class _StarGambitPlainGS:
    """StarGambit{Skirmish,Showdown,Clash,Battle}GS (star_gambit_gs.h:752-755): one configuration in its OWN action space
    (ActionSpace<Config>, :483-590) and its own 32-plane canonical form.  A view of the unified device game: actions map
    through to_unified_action (star_gambit_gs.cc:2522-2554), the planes are the 32 x D x D window of the canvas."""

    VARIANT = 0

    def __init__(self):
        self._u = StarGambitUnifiedGS(self.VARIANT)

    @classmethod
    def _dims(cls):
        side = 6 if cls.VARIANT == 3 else 5
        d = 2 * side + 1
        return side, d, d * d * 10

    @classmethod
    def NUM_PLAYERS(cls): return 2
    @classmethod
    def NUM_MOVES(cls): return cls._dims()[2] + 19
    @classmethod
    def CANONICAL_SHAPE(cls): return (32, cls._dims()[1], cls._dims()[1])
    @classmethod
    def POLICY_SHAPE(cls): return (10, cls._dims()[1], cls._dims()[1])
    @staticmethod
    def NUM_SYMMETRIES(): return 2

    def _to_unified(self, a):
        side, d, sp = self._dims()
        if self.VARIANT == 3:
            return a
        if a < sp:
            return ((a // 10 // d + 1) * 13 + (a // 10 % d + 1)) * 10 + a % 10
        return 1690 + (a - sp)

    def copy(self):
        g = self.__class__.__new__(self.__class__)
        g._u = self._u.copy()
        return g

    def __eq__(self, other): return isinstance(other, _StarGambitPlainGS) and self._u == other._u
    __hash__ = None
    def current_player(self): return self._u.current_player()
    def current_turn(self): return self._u.current_turn()
    def num_players(self): return 2
    def num_moves(self): return self.NUM_MOVES()
    def num_symmetries(self): return 2
    def relative_values(self): return True           # star_gambit_gs.h:628
    def randomize_start(self): return None
    def num_variants(self): return 0
    def get_variant_id(self): return -1
    def scores(self): return self._u.scores()
    def get_units(self): return self._u.get_units()
    def has_taken_action(self): return self._u.has_taken_action()
    def dump(self): return self._u.dump()
    __str__ = dump

    def valid_moves(self):
        side, d, sp = self._dims()
        uv = self._u.valid_moves()
        if self.VARIANT == 3:
            return uv
        out = np.zeros(sp + 19, np.uint8)
        out[:sp] = uv[:1690].reshape(13, 13, 10)[1:1 + d, 1:1 + d].reshape(-1)
        out[sp:] = uv[1690:]
        return out

    def play_move(self, move):
        move = int(move)
        if not 0 <= move < self.NUM_MOVES():
            raise RuntimeError(f"move {move} out of range")
        self._u.play_move(self._to_unified(move))

    def canonicalized(self):
        side, d, _ = self._dims()
        off = 0 if self.VARIANT == 3 else 1
        return self._u.canonicalized()[:32, off:off + d, off:off + d].copy()

    def to_bytes(self):                              # the inner image, star_gambit_gs.cc:2253-2288
        return self._u.to_bytes()[25:]

    @classmethod
    def from_bytes(cls, data):
        data = bytes(data)
        g = cls.__new__(cls)
        g._u = StarGambitUnifiedGS.from_bytes(struct.pack("<4fiBI", 0.25, 0.25, 0.25, 0.25, cls.VARIANT, cls.VARIANT, len(data)) + data)
        return g

    def __reduce__(self):
        return (_sg_from_bytes, (type(self).__name__, self.to_bytes()))


class StarGambitSkirmishGS(_StarGambitPlainGS): VARIANT = 0
class StarGambitShowdownGS(_StarGambitPlainGS): VARIANT = 1
class StarGambitClashGS(_StarGambitPlainGS): VARIANT = 2
class StarGambitBattleGS(_StarGambitPlainGS): VARIANT = 3
StarGambitGS = StarGambitSkirmishGS                   # the legacy name, star_gambit_gs.h:758


def _sg_from_bytes(name, data):
    return globals()[name].from_bytes(data)


def hash_game_state(gs):
    """hash_game_state(gs), game_state.h:141-156 / py_wrapper.cc:260-263: the 64-bit position key the caches use.  absl's
    hash is salted per process, so only equality semantics are contract; this is the engine's deterministic key over
    the same fields."""
    return int(gs._state()["key"][0])


def _init_rows(init, n):
    """start images of game_replay as one [n, stride] uint8 array: a list of bytes is zero-padded to the longest image"""
    if isinstance(init, np.ndarray):
        rows = np.ascontiguousarray(init, dtype=np.uint8)
        if rows.ndim != 2:
            raise RuntimeError(f"game_replay: init must be a list of bytes or a [n, stride] uint8 array, got shape {rows.shape}")
    else:
        images = [bytes(b) for b in init]
        rows = np.zeros((len(images), max((len(b) for b in images), default=0)), np.uint8)
        for i, b in enumerate(images):
            rows[i, :len(b)] = np.frombuffer(b, np.uint8)
    if rows.shape[0] != n:
        raise RuntimeError(f"game_replay: {rows.shape[0]} start positions for {n} move rows")
    return rows


def game_replay(game_cls, moves, init=None, device=0):
    """Batched rules replay on the device: moves [n, len] int32, -1 padded.  `init` = one start position per row
    (azmi_game_replay_from) as a list of bytes or a [n, stride] uint8 array of zero-padded rows: Connect4GS.to_bytes() images
    (89 bytes), _TaflBoardGS._image / to_bytes images; None = every row starts from the game's initial position
    (azmi_game_replay).  Moves are checked: a row with an illegal move gets status -1 and stops before it."""
    moves = np.ascontiguousarray(moves, dtype=np.int32)
    n, ln = moves.shape
    rows = None if init is None else _init_rows(init, n)
    P, M, chw = game_cls._info()
    out = dict(
        valid=np.zeros((n, M), np.uint8), scores=np.zeros((n, P + 1), np.float32),
        canonical=np.zeros((n,) + tuple(chw), np.float32), player=np.zeros(n, np.uint32),
        turn=np.zeros(n, np.uint32), key=np.zeros(n, np.uint64), status=np.zeros(n, np.int32),
    )
    if rows is None:
        check(lib.azmi_game_replay(game_cls.GAME_ID, device, moves.ctypes.data, n, ln, out["valid"].ctypes.data,
                                   out["scores"].ctypes.data, out["canonical"].ctypes.data, out["player"].ctypes.data,
                                   out["turn"].ctypes.data, out["key"].ctypes.data, out["status"].ctypes.data))
    else:
        check(lib.azmi_game_replay_from(game_cls.GAME_ID, device, rows.ctypes.data, rows.shape[1], moves.ctypes.data, n, ln,
                                        out["valid"].ctypes.data, out["scores"].ctypes.data, out["canonical"].ctypes.data,
                                        out["player"].ctypes.data, out["turn"].ctypes.data, out["key"].ctypes.data,
                                        out["status"].ctypes.data))
    return out
