"""
The device's subsequence path of Motion-JPEG entropy decoding restated in plain Python (csrc/jpeg_decode_kernels.hpp, 1b, holds the
definition; tests/jpeg_ref.py the serial decoder whose coefficients it must give): the lanes of a staged frame, a lane's decode from an
entry state to an exit state, the synchronisation rounds, the segmented scan and the write pass.

A state is (byte, bit, b, k) — where the next symbol starts (the byte's offset in the scan, never the 00 of a stuffed FF 00) and what it
is (block b of the MCU, zigzag index k; k = 0: a DC size) — or None (invalid: a lane that is entered so decodes from its assumed entry). `rounds` counts Jacobi rounds over the whole frame: in
round r every lane takes the exit its predecessor had after round r - 1 and decodes again when that is not the entry it last used;
the count is the number of rounds in which some lane did. After it the entries are the predecessors' exits (the fixed point), and the
states are the serial decoder's by induction from the intervals' known entries. `settles` restates the device's two phases of rounds
inside workgroups instead, for the claim that a frame whose Jacobi count is within the budget does not fall back.
"""
from __future__ import annotations

import bisect
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent))
import jpeg_ref as J  # noqa: E402

GROUP = 256                                                           # JPEG_SYNC_LANES
SIZES = (8, 16, 64)
# Jacobi rounds of every stream of tests/golden/jpeg_streams.npz at subsequences of 8, 16 and 64 bytes (tests/test_host_mjpeg_sync.py
# holds them to `decode`): what a round budget has to cover for the device not to fall back
ROUNDS = {
    "long_420": (293, 191, 39), "long_grey": (8, 5, 2), "mid_420": (75, 34, 9), "mid_444": (46, 23, 6), "no_dht_420": (85, 42, 10),
    "odd_420": (55, 27, 7), "odd_422": (43, 22, 6), "odd_grey": (19, 9, 2), "one_mcu_420": (28, 14, 3), "one_mcu_444": (5, 1, 0),
    "own_extremes": (166, 83, 20), "own_sparse": (9, 5, 1), "partial_420": (27, 13, 3), "partial_422": (19, 9, 3), "partial_444": (5, 2, 0),
    "tall_420": (30, 15, 4), "tall_444": (21, 9, 2), "wide_420": (85, 42, 10), "wide_422": (15, 9, 2),
}


class Frame:
    """A stream as the device sees it: the staged frame's words (mjpegsource.stage), its scan, tables and geometry"""

    def __init__(self, stream: bytes):
        from shaderflow_amd import mjpegsource as M
        header = M.parse_header(stream)
        view = np.zeros(M.capacity_for(header, len(stream)), np.uint8)
        total = M.stage(stream, header, view)
        fixed = view[:M.FRAME_FIXED].view(M.STAGED)[0]
        self.header = header
        self.intervals, self.restart, self.scan_bytes = int(fixed["intervals"]), int(fixed["restart"]), int(fixed["scan_bytes"])
        self.offsets = [int(v) for v in view[M.FRAME_FIXED:M.FRAME_FIXED + 4*self.intervals].view("<u4")]
        self.scan = bytes(view[int(fixed["scan_offset"]):total])
        assert len(self.scan) == self.scan_bytes
        h, v = header.sampling
        self.luma_blocks = 1 if header.components == 1 else h*v
        self.blocks = 1 if header.components == 1 else h*v + 2
        self.mcus = header.mcus
        self.lookups = {key: {pair: symbol for symbol, pair in J.huffman_codes(list(bits), list(values)).items()} for key, (bits, values) in header.huffman.items()}
        self.pieces: dict = {}
        self.fast: dict = {}

    def bounds(self, interval: int) -> tuple[int, int]:
        finish = self.offsets[interval + 1] if interval + 1 < self.intervals else self.scan_bytes + 2
        return self.offsets[interval], finish - 2

    def slots(self, interval: int) -> int:
        return min(self.restart, self.mcus - interval*self.restart)*self.blocks*64

    def logical(self, interval: int) -> tuple:
        """The interval's bytes without the stuffed zeros: their values (four zero bytes behind them, as the device's reader feeds
        zero bits past the end), their offsets in the scan, and where the data ends (the interval's end, or a marker inside it)"""
        if interval not in self.pieces:
            begin, end = self.bounds(interval)
            values, where, p = bytearray(), [], begin
            while p < end:
                byte = self.scan[p]
                if byte != 0xff:
                    values.append(byte), where.append(p)
                    p += 1
                elif p + 1 < end and self.scan[p + 1] == 0:
                    values.append(byte), where.append(p)
                    p += 2
                else:
                    break
            self.pieces[interval] = (bytes(values) + bytes(8), where, p, {address: n for n, address in enumerate(where)})
        return self.pieces[interval]

    def table(self, kind: int, selector: int) -> tuple:
        """(the first 8 bits → (length, symbol) or None, (code, length) → symbol)"""
        key = (kind, selector)
        if key not in self.fast:
            lookup, first = self.lookups[key], [None]*256
            for (code, length), symbol in lookup.items():
                if length <= 8:
                    for rest in range(1 << (8 - length)):
                        first[(code << (8 - length)) | rest] = (length, symbol)
            self.fast[key] = (first, lookup)
        return self.fast[key]


def lanes_of(frame: Frame, subsequence: int) -> list:
    """Every lane of the frame: None (idle) or (interval, lo, hi, head, last); lane offsets[i]//S + i + t is interval i's piece t"""
    count = -(-frame.scan_bytes//subsequence) + frame.intervals
    lanes: list = [None]*count
    for interval in range(frame.intervals):
        begin, end = frame.bounds(interval)

        def moved(a):
            return a + 1 if begin < a < end and frame.scan[a - 1] == 0xff and frame.scan[a] == 0 else a
        piece = 0
        while True:
            cut = begin if piece == 0 else (begin//subsequence + piece)*subsequence
            if cut >= end:
                break
            following = (begin//subsequence + piece + 1)*subsequence
            last = following >= end
            index = begin//subsequence + interval + piece
            assert lanes[index] is None
            lanes[index] = (interval, moved(cut), end if last else moved(following), piece == 0, last)
            piece += 1
    return lanes


def decode_piece(frame: Frame, lane: tuple, entry, out=None, first: int = 0, predictors=(0, 0, 0)):
    """A lane from `entry` → (exit, slots, [DC sums], error). With `out` (the interval's slots, the write pass): stores from slot
    `first` on and stops at the interval's last slot; `error` names what went wrong (None: nothing)."""
    interval, lo, hi, _, _ = lane
    if entry is None:
        if out is not None:
            return None, 0, [0, 0, 0], None                           # the write pass: the lane in front met a real error
        entry = (lo, 0, 0, 0)                                         # the rounds: the lane in front ran into nonsense; assume again
    byte, bit, b, k = entry
    if byte >= hi:
        return entry, 0, [0, 0, 0], None                               # entered beyond its own end
    values, where, data_end, at = frame.logical(interval)
    assert byte >= lo and byte in at
    position = at[byte]*8 + bit
    inside = bisect.bisect_left(where, hi)                              # logical bytes of the interval in front of the piece's end
    limit, available = inside*8, len(where)*8
    total = len(out) if out is not None else None
    slot, sums, error = first, [0, 0, 0], None
    tables = [(frame.table(0, td), frame.table(1, ta)) for _, td, ta in frame.header.selectors]

    def peek(count):                                                    # the next `count` ≤ 16 bits
        n = position >> 3
        return (int.from_bytes(values[n:n + 4], "big") >> (32 - count - (position & 7))) & ((1 << count) - 1)

    while position < limit and not (out is not None and slot >= total):
        component = 0 if b < frame.luma_blocks else b - frame.luma_blocks + 1
        quick, lookup = tables[component][0 if k == 0 else 1]
        code = peek(16)
        found = quick[code >> 8]
        if found is None:
            for length in range(9, 17):
                if (code >> (16 - length), length) in lookup:
                    found = (length, lookup[(code >> (16 - length), length)])
                    break
        if found is None:
            error = "code"
            break
        position += found[0]
        symbol = found[1]
        if k == 0:
            if symbol > 15:
                error = "code"
                break
            sums[component] += J.extend(peek(symbol), symbol) if symbol else 0
            position += symbol
            if out is not None and slot < total:
                out[slot] = predictors[component] + sums[component]
            slot, k = slot + 1, 1
        else:
            run, size = symbol >> 4, symbol & 15
            if size == 0:
                count = 64 - k if run != 15 else 16
                if k + count > 64:
                    error = "run"
                    break
                if out is not None:
                    out[slot:min(slot + count, total)] = 0
                slot, k = slot + count, k + count
            else:
                if k + run > 63:
                    error = "run"
                    break
                if out is not None:
                    out[slot:min(slot + run, total)] = 0
                    if slot + run < total:
                        out[slot + run] = J.extend(peek(size), size)
                position += size
                slot, k = slot + run + 1, k + run + 1
        if k >= 64:
            k, b = 0, (b + 1) % frame.blocks
        if position > available:
            error = "bits"
            break
    if error:
        return None, slot - first, sums, error
    n = position >> 3
    return (where[n] if n < len(where) else data_end, position & 7, b, k), slot - first, sums, None


class Sync:
    """The records of one frame at one subsequence size"""

    def __init__(self, frame: Frame, subsequence: int):
        self.frame, self.lanes = frame, lanes_of(frame, subsequence)
        self.entry: list = [None]*len(self.lanes)
        self.result: list = [None]*len(self.lanes)
        for n, lane in enumerate(self.lanes):
            if lane is not None:
                self.entry[n] = (lane[1], 0, 0, 0)                      # known for a head, assumed for the others
                self.result[n] = decode_piece(frame, lane, self.entry[n])

    def exit(self, n):
        return self.result[n][0]

    def take(self, n, want) -> bool:
        """Lane n decodes again if `want` is not the entry it last used"""
        lane = self.lanes[n]
        if lane is None or lane[3] or want == self.entry[n]:
            return False
        self.entry[n] = want
        self.result[n] = decode_piece(self.frame, lane, want)
        return True

    def jacobi(self, limit: int = 1 << 20) -> int:
        rounds = 0
        while rounds < limit:
            exits = [self.exit(n) if self.lanes[n] is not None else None for n in range(len(self.lanes))]
            changed = [self.take(n, exits[n - 1]) for n in range(1, len(self.lanes))]
            if not any(changed):
                break
            rounds += 1
        return rounds

    def chains(self) -> int:
        """jacobi()'s count and end state without its rounds. The exit of lane i after round r is the state of the chain that starts at
        lane i - r with the assumed entry (or at the interval's head, with the known one) and runs through lane i; so lane i decodes
        again in round r exactly when the chains from lane i - r and from lane i - r + 1 enter it in different states. Chains that
        meet in one state at one lane stay together: every (lane, entry) pair is decoded once, the chains are paths over these nodes,
        and the count is the longest stretch over which two neighbouring chains stay apart."""
        nodes: dict = {}                                               # (lane, entry) → [result, the next node's key]
        rounds = 0
        for head in [n for n, lane in enumerate(self.lanes) if lane is not None and lane[3]]:
            last = head
            while not self.lanes[last][4]:
                last += 1
            for start in range(last, head - 1, -1):
                key = (start, (self.lanes[start][1], 0, 0, 0))
                while key not in nodes:
                    n, entry = key
                    result = decode_piece(self.frame, self.lanes[n], entry)
                    following = (n + 1, result[0]) if n < last else None
                    nodes[key] = (result, following)
                    if following is None:
                        break
                    key = following
            for start in range(head, last):
                a, b = nodes[(start, (self.lanes[start][1], 0, 0, 0))][1], (start + 1, (self.lanes[start + 1][1], 0, 0, 0))
                apart = 0
                while a is not None and a != b:
                    apart += 1
                    a, b = nodes[a][1], nodes[b][1]
                rounds = max(rounds, apart)
            key = (head, (self.lanes[head][1], 0, 0, 0))
            while key is not None:
                self.entry[key[0]] = key[1]
                self.result[key[0]], key = nodes[key]
        return rounds

    def phases(self, budget: int) -> None:
        """The device's rounds: inside workgroups of GROUP lanes, twice, the second time with the hand-over between them"""
        groups = range(0, len(self.lanes), GROUP)
        count = 2 if len(self.lanes) > GROUP and budget > 0 else 1
        for phase in range(count):
            handoff = [self.exit(n - 1) if self.lanes[n - 1] is not None else None for n in groups]
            for g, base in enumerate(groups):
                members = range(base, min(base + GROUP, len(self.lanes)))
                for r in range(budget):
                    exits = {n: (self.exit(n) if self.lanes[n] is not None else None) for n in members}
                    changed = False
                    for n in members:
                        if n > base:
                            changed |= self.take(n, exits[n - 1])
                        elif phase == 1 and r == 0 and g > 0:
                            changed |= self.take(n, handoff[g])
                    if not changed:
                        break

    def settled(self) -> bool:
        return all(lane is None or lane[3] or self.entry[n] == self.exit(n - 1) for n, lane in enumerate(self.lanes))

    def write(self) -> tuple[np.ndarray, list]:
        """The scan and the write pass → coefficients (mcus, blocks, 64) and the errors met"""
        frame = self.frame
        out = np.zeros(frame.mcus*frame.blocks*64, np.int64)
        errors, first, predictors = [], 0, [0, 0, 0]
        for n, lane in enumerate(self.lanes):
            if lane is None:
                continue
            interval = lane[0]
            if lane[3]:
                first, predictors = 0, [0, 0, 0]
            base, total = interval*frame.restart*frame.blocks*64, frame.slots(interval)
            _, slots, _, error = decode_piece(frame, lane, self.entry[n], out[base:base + total], first, tuple(predictors))
            if error and first + slots < total:
                errors.append((n, error))
            elif lane[4] and first + slots < total:
                errors.append((n, "short"))
            first += self.result[n][1]
            predictors = [a + b for a, b in zip(predictors, self.result[n][2])]
        return out.reshape(frame.mcus, frame.blocks, 64), errors


def decode(stream: bytes, subsequence: int, budget: int | None = None) -> dict:
    """{"coefficients", "rounds" (Jacobi rounds to the fixed point), "subsequences", "errors"}; with `budget`: the device's phases instead,
    and "fell_back" when they did not settle (the coefficients are then not written: None)"""
    frame = Frame(stream)
    sync = Sync(frame, subsequence)
    info = {"subsequences": len(sync.lanes), "frame": frame}
    if budget is None:
        info["rounds"] = sync.chains()
        assert sync.settled()
    else:
        sync.phases(min(budget, GROUP - 1))
        info["fell_back"] = not sync.settled()
        if info["fell_back"]:
            return {**info, "coefficients": None, "errors": []}
    info["coefficients"], info["errors"] = sync.write()
    return info


def pillow_noise() -> bytes:
    """A 128 x 96 noise picture as Pillow writes it at quality 90: 4:2:0, the standard's tables, no DRI segment — one interval"""
    import io

    from PIL import Image
    buffer = io.BytesIO()
    Image.fromarray(J.picture("noise", 128, 96, 5)).save(buffer, "JPEG", quality=90)
    return buffer.getvalue()


def golden_streams() -> dict:
    data = np.load(Path(__file__).resolve().parent/"golden"/"jpeg_streams.npz")
    return {name[:-7]: data[name].tobytes() for name in data.files if name.endswith(".stream")}
