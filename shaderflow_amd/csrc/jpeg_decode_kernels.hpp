// jpeg_decode_kernels.hpp — baseline JPEG frames of a Motion-JPEG source on the device (capi_video.hip launches these):
// the inverse of jpeg_kernels.hpp, for streams other encoders wrote as well as this project's own.
//
// The decode is DEFINED here and restated in float64 by tests/jpeg_decode_ref.py:
//   * input: baseline sequential (SOF0), 8 bit, Huffman, ONE interleaved scan; three components read as JFIF YCbCr with luma sampling
//     2x2 (4:2:0), 2x1 (4:2:2) or 1x1 (4:4:4) and chroma 1x1, or one component (grey); 8-bit quantisation tables; the stream's own
//     Huffman tables (the host puts the standard's Annex K tables in their place when the stream has no DHT); any restart interval,
//     RSTn checked modulo 8. Everything else is refused by the host's header parser (mjpegsource.py) before a byte is staged;
//   * entropy decoding: the unit is the restart interval (the DC predictors are zero at its start, nothing crosses intervals). A
//     stream without restart markers is one interval. Short intervals take a lane each (1 below); long ones are cut into subsequences
//     with a lane each (1b below) — the same coefficients, value for value;
//   * samples: coefficient times its quantiser (integers), 8 x 8 inverse DCT in f32 with the encoder's orthonormal basis
//     (dct[u][x] = C(u)/2 cos((2x + 1) u pi / 16)): along the rows first, tmp[v][x] = sum over u = 0…7 of F[v][u] dct[u][x], then down
//     the columns, s[y][x] = sum over v = 0…7 of tmp[v][x] dct[v][y], both as fma chains in that order; add 128, round half up
//     (floor(s + 128 + 0.5)), clip to 0…255;
//   * chroma upsampling: the centred triangle filter in integers, edges replicated at the component's OWN extent ceil(w h_c / h_max)
//     (rows alike), not at the MCU padding:
//       2x1: even output (3 c[j] + c[j-1] + 1) >> 2, odd output (3 c[j] + c[j+1] + 2) >> 2;
//       2x2: column sums s = 3 near_row + far_row (the far row is the one above for an even output row, below for an odd one),
//            even output (3 s[j] + s[j-1] + 8) >> 4, odd output (3 s[j] + s[j+1] + 7) >> 4;
//   * colour, full range, 16-bit fixed point, arithmetic shifts, Cb' = Cb - 128, Cr' = Cr - 128, each clipped to 0…255:
//       R = Y + (( 91881 Cr' + 32768) >> 16)
//       G = Y + ((-22554 Cb' - 46802 Cr' + 32768) >> 16)
//       B = Y + ((116130 Cb' + 32768) >> 16)                         grey: R = G = B = Y;
//   * output: the module's RGB8 texture, rows bottom-up, exactly as k_video_frame writes it.
//
// A staged frame (what the host's reader puts into a slot) is `sfx_jpeg_frame` (include/shaderflow_hip.h: the six words, the components'
// table selectors, four quantisation tables in zigzag order, four Huffman tables as BITS and HUFFVAL), one word per restart interval
// behind it (the host's reader finds the FF D0…D7 pairs with numpy: DESIGN.md §7c says why), then, 16-byte aligned, the scan.
// The host validates the words when a frame is submitted (capi_video.hip); the kernels check them again and clamp what they index with.
//
// The kernels, on the render stream:
//   k_jpeg_sync_*          frames with long intervals: a lane per subsequence, in rounds, a scan and a write pass (1b below has the text);
//   k_jpeg_decode_entropy  a lane per restart interval (a wave serves 64 of them), one launch per staged frame: the Huffman lookups are built
//                          in LDS from the frame's own tables, the int16 coefficients leave in zigzag order, MCU by MCU (the encoder's
//                          layout). Every read is bounded by the interval's end and every loop by 64 terms and the interval's MCU count.
//                          A code that matches nothing, a run past 63, a missing or wrong RSTn and bits running out set bits of the
//                          frame's status word — never a fault, never a write outside the frame's scratch;
//   k_jpeg_decode_planes   dequantisation and the inverse DCT through LDS, four blocks per workgroup → the components' 8-bit planes;
//   k_jpeg_decode_pixels   upsampling, colour, row flip, RGB8 stores: a lane per run of 16 pixels, 16-byte aligned stores when the row
//                          pitch allows, heads and tails as k_video_frame's planar path has them.
// The pixel stage is two launches, not one: the triangle filter reads a ring of samples of the eight neighbouring chroma blocks, and a
// fused kernel would transform those blocks again per MCU (3.7 times the arithmetic at 4:2:0) to save 1.5 bytes per pixel written and
// read once (counted, not measured: DESIGN.md §7c).
#pragma once

#include "jpeg_common.hpp"

namespace sf {

constexpr int JPEG_FRAME_FIXED = sizeof(sfx_jpeg_frame);               // the interval table starts here

struct JpegDecodeGeometry {
    int width, height;
    int components;                 // 3 (YCbCr) or 1 (grey)
    int hs, vs;                     // luma sampling factors: 2x2, 2x1 or 1x1 (chroma, and grey, 1x1)
    int mcus_x, mcus_y, blocks;     // MCUs per row, MCU rows, blocks per MCU (hs*vs + 2, or 1)
    int capacity;                   // bytes of a staged frame at the most
};

inline size_t jpeg_decode_coefficients(const JpegDecodeGeometry& g) { return (size_t)g.mcus_x*g.mcus_y*g.blocks*64; }
__host__ __device__ inline size_t jpeg_plane_offset(const JpegDecodeGeometry& g, int component) {
    const size_t luma = (size_t)g.mcus_x*g.hs*8*g.mcus_y*g.vs*8, chroma = (size_t)g.mcus_x*8*g.mcus_y*8;
    return component == 0 ? 0 : luma + (component - 1)*chroma;
}
inline size_t jpeg_plane_bytes(const JpegDecodeGeometry& g) { return jpeg_plane_offset(g, g.components); }

// ---- 1. Huffman decoding, a lane per restart interval ------------------------------------------------------------------------------
// The bit reader keeps up to 64 bits, right-aligned. Past the interval's end, or at a marker inside it, it feeds zero bits and counts
// them (`fake`): they sit below the real ones, so real bits have run out exactly when fewer than `fake` bits are left.
struct JpegBitReader {
    const uint8_t* p; const uint8_t* end;
    unsigned long long acc; int n, fake;
};

__device__ __forceinline__ void jpeg_fill(JpegBitReader& r) {         // afterwards at least 57 bits are there
    while (r.n <= 56) {
        uint32_t byte = 0; bool real = false;
        if (r.p < r.end) {
            byte = *r.p;
            if (byte != 0xffu) { r.p++; real = true; }
            else if (r.p + 1 < r.end && r.p[1] == 0) { r.p += 2; real = true; }      // a stuffed FF
            else { r.end = r.p; byte = 0; }                              // a marker, or an FF the interval ends in: the data ends here
        }
        if (!real) r.fake += 8;
        r.acc = (r.acc << 8) | byte; r.n += 8;
    }
}
__device__ __forceinline__ int jpeg_take(JpegBitReader& r, int count) { // count ≤ 16 ≤ r.n
    r.n -= count;
    return (int)((r.acc >> r.n) & ((1ull << count) - 1ull));
}
__device__ __forceinline__ int jpeg_extend(int value, int size) { return (size == 0 || value >= (1 << (size - 1))) ? value : value - (1 << size) + 1; }
// whether interval `interval`'s bytes [begin, finish - 2) lie in the scan and its RSTn marker stands in front of them: 0, or SFX_JPEG_BAD_RESTART
__device__ __forceinline__ uint32_t jpeg_interval_fault(const uint8_t* scan, uint32_t scan_bytes, uint32_t interval, unsigned long long begin, unsigned long long finish) {
    if (begin > scan_bytes || finish < begin + 2ull || finish > (unsigned long long)scan_bytes + 2ull) return SFX_JPEG_BAD_RESTART;      // this interval's marker, or the next one's, is missing
    if (interval > 0u && (begin < 2ull || scan[begin - 2] != 0xffu || scan[begin - 1] != 0xd0u + ((interval - 1u) & 7u))) return SFX_JPEG_BAD_RESTART;
    return 0u;
}

// The Huffman lookups of a frame's four tables (0, 1: DC; 2, 3: AC), built in LDS by every workgroup that decodes
struct JpegHuffmanLookup {
    uint16_t lookup[4][256];                                            // the next 8 bits → (length << 8) | symbol; 0: a longer code, or none
    int maxcode[4][17], valoff[4][17];                                  // Annex F.2.2.3: the largest code of each length (-1: none), VALPTR - MINCODE
    uint8_t values[4][256];
};
__device__ __forceinline__ void jpeg_build_lookup(JpegHuffmanLookup& h, const sfx_jpeg_frame& f, int lane, int lanes) {   // the whole workgroup calls it
    for (int k = lane; k < 4*256; k += lanes) h.values[k >> 8][k & 255] = f.huffman[k >> 8].values[k & 255];
    if (lane < 4) {
        const uint8_t* bits = f.huffman[lane].bits;
        int code = 0, first = 0;
        for (int length = 1; length <= 16; length++) {
            const int count = bits[length - 1];
            h.valoff[lane][length] = first - code;
            h.maxcode[lane][length] = count ? code + count - 1 : -1;
            first += count; code = (code + count) << 1;
        }
    }
    __syncthreads();
    for (int k = lane; k < 4*256; k += lanes) {
        const int table = k >> 8, peek = k & 255;
        uint32_t entry = 0;
        for (int length = 1; length <= 8; length++) {
            const int code = peek >> (8 - length);
            if (code <= h.maxcode[table][length]) {
                const int at = h.valoff[table][length] + code;
                if (at >= 0 && at < 256) entry = ((uint32_t)length << 8) | h.values[table][at];
                break;
            }
        }
        h.lookup[table][peek] = (uint16_t)entry;
    }
    __syncthreads();
}
// one Huffman symbol of table `table`; -1 when no code matches
__device__ __forceinline__ int jpeg_symbol(JpegBitReader& reader, const JpegHuffmanLookup& h, int table) {
    jpeg_fill(reader);
    const int peek = (int)((reader.acc >> (reader.n - 16)) & 0xffffull);
    const uint32_t entry = h.lookup[table][peek >> 8];
    if (entry) { reader.n -= (int)(entry >> 8); return (int)(entry & 255u); }
    for (int length = 1; length <= 16; length++) {
        const int code = peek >> (16 - length);
        if (code <= h.maxcode[table][length]) {
            const int at = h.valoff[table][length] + code;
            if (at < 0 || at >= 256) return -1;
            reader.n -= length;
            return h.values[table][at];
        }
    }
    return -1;
}

// `only_if`: null, or a word of the subsequence path's (1b below): the kernel returns at once unless it is set — the fall-back's launch
__global__ void __launch_bounds__(64) k_jpeg_decode_entropy(const uint8_t* __restrict__ frame, int16_t* __restrict__ coefficients, uint32_t* __restrict__ status,
                                                            JpegDecodeGeometry g, const uint32_t* __restrict__ only_if) {
    __shared__ JpegHuffmanLookup tables;
    if (only_if && *only_if == 0u) return;                              // (uniform)
    const int lane = threadIdx.x;
    const sfx_jpeg_frame& f = *reinterpret_cast<const sfx_jpeg_frame*>(frame);
    const uint32_t scan_bytes = f.scan_bytes, restart = f.restart, intervals = f.intervals, scan_offset = f.scan_offset;
    const unsigned long long total = (unsigned long long)g.mcus_x*g.mcus_y;
    const bool sane = jpeg_descriptor_fault(f, g.mcus_x, g.mcus_y, (unsigned long long)g.capacity) == 0;
    if (!sane) {                                                        // (uniform: the whole workgroup leaves)
        if (blockIdx.x == 0 && lane == 0) atomicOr(status, SFX_JPEG_BAD_DESCRIPTOR);
        return;
    }
    jpeg_build_lookup(tables, f, lane, 64);

    const uint32_t interval = blockIdx.x*64u + (uint32_t)lane;
    if (interval >= intervals) return;
    const uint32_t* offsets = reinterpret_cast<const uint32_t*>(frame + JPEG_FRAME_FIXED);
    const uint8_t* scan = frame + scan_offset;
    const unsigned long long begin = offsets[interval], finish = interval + 1u < intervals ? (unsigned long long)offsets[interval + 1u] : (unsigned long long)scan_bytes + 2ull;
    uint32_t flags = jpeg_interval_fault(scan, scan_bytes, interval, begin, finish);
    if (flags) { atomicOr(status, flags); return; }

    JpegBitReader reader{scan + begin, scan + (finish - 2ull), 0ull, 0, 0};
    const int luma_blocks = g.components == 1 ? 1 : g.hs*g.vs;
    const unsigned long long first_mcu = (unsigned long long)interval*restart;
    const int mcus = (int)(total - first_mcu < restart ? total - first_mcu : restart);
    int16_t* out = coefficients + (size_t)first_mcu*g.blocks*64;
    int predictor0 = 0, predictor1 = 0, predictor2 = 0;

    for (int m = 0; m < mcus && !flags; m++) {
        for (int b = 0; b < g.blocks && !flags; b++, out += 64) {
            const int component = b < luma_blocks ? 0 : b - luma_blocks + 1;
            const int dc_table = f.td[component] & 1, ac_table = 2 + (f.ta[component] & 1);
            for (int k = 0; k < 8; k++) reinterpret_cast<uint4*>(out)[k] = make_uint4(0u, 0u, 0u, 0u);
            int size = jpeg_symbol(reader, tables, dc_table);
            if (size < 0 || size > 15) { flags |= SFX_JPEG_BAD_CODE; break; }
            const int difference = jpeg_extend(jpeg_take(reader, size), size);
            int& predictor = component == 0 ? predictor0 : (component == 1 ? predictor1 : predictor2);
            predictor += difference;
            out[0] = (int16_t)predictor;
            int k = 1;
            for (int term = 0; term < 64 && k < 64; term++) {
                const int code = jpeg_symbol(reader, tables, ac_table);
                if (code < 0) { flags |= SFX_JPEG_BAD_CODE; break; }
                const int run = code >> 4;
                size = code & 15;
                if (size == 0) {
                    if (run != 15) break;                               // EOB
                    k += 16;
                    if (k > 64) { flags |= SFX_JPEG_BAD_RUN; break; }
                    continue;
                }
                k += run;
                if (k > 63) { flags |= SFX_JPEG_BAD_RUN; break; }
                out[k++] = (int16_t)jpeg_extend(jpeg_take(reader, size), size);
            }
            if (reader.n < reader.fake) flags |= SFX_JPEG_OUT_OF_BITS;
        }
    }
    if (flags) atomicOr(status, flags);
}

// ---- 1b. Huffman decoding, a lane per subsequence (self-synchronising: Weißenberger & Schmidt) ------------------------------
// For frames whose restart intervals are long (a stream without restart markers is ONE interval). DEFINED here, restated in Python by
// tests/jpeg_sync_ref.py; the coefficients are k_jpeg_decode_entropy's, value for value.
//   * subsequences: the scan is cut at every multiple of S bytes (counted from the scan's start) and at every interval's start. Interval
//     i's piece t (t = 0, 1, …) is lane offsets[i]/S + i + t of the frame: lane numbers follow from the interval table by arithmetic, a
//     lane finds its interval by a bounded binary search, and a frame has at most ceil(scan_bytes/S) + intervals lanes (some stay idle:
//     where a marker straddles a cut). A cut that falls on the 00 of a stuffed FF 00 moves one byte on, for both lanes it parts;
//   * a state is (byte, bit, block b of the MCU, zigzag index k, valid): where the next symbol starts and what it is (k = 0: a DC size).
//     A lane decodes the symbols that START inside its piece, from an entry state to an exit state, and counts the coefficient slots it
//     passes (a DC value 1, an AC value run + 1, ZRL 16, EOB 64 - k) and the DC differences per component. A code that matches nothing,
//     a run past 63 or bits running out make the exit invalid. An entry beyond the piece's end is passed on unchanged. A lane that is
//     entered with an invalid state decodes from its assumed entry again (the chain in front of it ran into nonsense: a new one starts
//     here), except in the write pass, where it does nothing: there the lane in front has met a real error and reported it;
//   * k_jpeg_sync_rounds, phase 0: every lane decodes from the assumed entry (its first byte, bit 0, b = 0, k = 0), an interval's first
//     lane from the known one. Then rounds inside the workgroup (256 lanes): a lane whose predecessor's exit is not the entry it last
//     used decodes again from it. At most `budget` rounds, fewer when a round changes nothing. Phase 1 (a second launch, when the frame
//     has more than one workgroup): a workgroup's first lane takes the exit the workgroup in front of it left in phase 0, then rounds
//     as before. Nothing is written to the coefficients;
//   * k_jpeg_sync_scan (one workgroup): a segmented exclusive prefix sum over the records, cut at interval starts → every lane's first
//     slot and its three DC predictors; and the test of the fixed point: every lane's entry IS its predecessor's exit. Then, by
//     induction from the intervals' known entries, every state is the serial decoder's: exact, not probable. If not (the budget was
//     too small), `control[0]` is set;
//   * k_jpeg_sync_write: every lane decodes once more and stores: coefficients, zeros for the slots it passes, final DC values. It
//     stores slots [first, first + count) of its interval's own range only, and stops at the interval's last slot. Errors are real
//     here and set the frame's status: SFX_JPEG_BAD_CODE, SFX_JPEG_BAD_RUN, SFX_JPEG_OUT_OF_BITS (also: an interval whose lanes end
//     short of mcus x blocks x 64 slots), SFX_JPEG_BAD_RESTART (thread n of the launch checks interval n as k_jpeg_decode_entropy does).
//     With `control[0]` set it leaves the frame alone, and k_jpeg_decode_entropy, launched behind it with `only_if` = control, decodes.
// Every loop is bounded before it starts: a piece's decode by its bit count (a symbol takes at least one bit), the rounds by the budget,
// the scan by the record count, the search by 32 halvings. No workgroup waits for another inside a launch.
constexpr int JPEG_SYNC_LANES = 256;                                    // lanes of a workgroup: round budgets stay below it (see capi_video.hip)
constexpr uint32_t JPEG_SYNC_VALID = 1u << 24, JPEG_SYNC_HEAD = 1u << 25, JPEG_SYNC_IDLE = 1u << 26;

struct JpegSyncRecord {                                                 // 64 bytes per lane
    uint2 entry, exit;              // states: x = byte (from the scan's start), y = bit | b << 8 | k << 16 | JPEG_SYNC_VALID
    uint32_t slots, dc[3];          // what the lane passed from `entry` to `exit`
    uint32_t flags;                 // JPEG_SYNC_HEAD: an interval's first lane; JPEG_SYNC_IDLE: no piece
    uint32_t first[2], predictor[3];// the scan's: the lane's first slot in its interval (64 bit), the DC predictors in front of it
    uint32_t unused[2];
};
static_assert(sizeof(JpegSyncRecord) == 64, "a record is 64 bytes");
struct JpegSyncScratch {
    JpegSyncRecord* records;        // `capacity` of them
    uint2* handoff;                 // per workgroup: its last lane's exit after phase 0
    uint32_t* rounds;               // per workgroup and phase: rounds that changed something
    uint32_t* control;              // [0] the fixed point was not reached (the fall-back decodes), [1] rounds used, [2] subsequences
    uint32_t capacity;
};
__host__ __device__ inline unsigned long long jpeg_sync_lanes(unsigned long long scan_bytes, unsigned long long intervals, unsigned long long subsequence) {
    return (scan_bytes + subsequence - 1ull)/subsequence + intervals;
}
// whether the frame's words allow the subsequence path with this launch: the descriptor is sane, its lanes fit the launch and the records
__device__ __forceinline__ bool jpeg_sync_sane(const sfx_jpeg_frame& f, const JpegDecodeGeometry& g, const JpegSyncScratch& s, uint32_t subsequence, unsigned long long launched) {
    if (subsequence < 2u || jpeg_descriptor_fault(f, g.mcus_x, g.mcus_y, (unsigned long long)g.capacity) != 0) return false;
    const unsigned long long lanes = jpeg_sync_lanes(f.scan_bytes, f.intervals, subsequence);
    return lanes <= launched && lanes <= s.capacity;
}

struct JpegSyncLane {
    uint32_t flags;                 // JPEG_SYNC_HEAD, JPEG_SYNC_IDLE
    uint32_t interval;
    uint32_t lo, hi, end;           // the piece [lo, hi) and the interval's last byte + 1, from the scan's start
    bool last;                      // the interval's last piece
};
__device__ __forceinline__ JpegSyncLane jpeg_sync_lane(const uint8_t* frame, const sfx_jpeg_frame& f, uint32_t subsequence, unsigned long long lane) {
    const uint32_t* offsets = reinterpret_cast<const uint32_t*>(frame + JPEG_FRAME_FIXED);
    const uint8_t* scan = frame + f.scan_offset;
    const uint32_t intervals = f.intervals, scan_bytes = f.scan_bytes;
    JpegSyncLane out{JPEG_SYNC_IDLE, 0u, 0u, 0u, 0u, false};
    uint32_t low = 0u, high = intervals - 1u;                           // the last interval whose first lane is not behind this one
    for (int step = 0; step < 32 && low < high; step++) {
        const uint32_t middle = low + (high - low + 1u)/2u;
        if ((unsigned long long)(offsets[middle]/subsequence) + middle <= lane) low = middle; else high = middle - 1u;
    }
    const unsigned long long begin = offsets[low], finish = low + 1u < intervals ? (unsigned long long)offsets[low + 1u] : (unsigned long long)scan_bytes + 2ull;
    if (begin > scan_bytes || finish < begin + 2ull || finish > (unsigned long long)scan_bytes + 2ull) return out;    // (k_jpeg_sync_write reports it)
    const unsigned long long first = begin/subsequence + low;
    if (lane < first) return out;
    const unsigned long long piece = lane - first, end = finish - 2ull;
    const unsigned long long cut = piece == 0ull ? begin : (begin/subsequence + piece)*subsequence;
    if (cut >= end) return out;
    const unsigned long long next = (begin/subsequence + piece + 1ull)*subsequence;
    auto moved = [&](unsigned long long a) { return (a > begin && a < end && scan[a - 1ull] == 0xffu && scan[a] == 0u) ? a + 1ull : a; };
    out.flags = piece == 0ull ? JPEG_SYNC_HEAD : 0u;
    out.interval = low;
    out.lo = (uint32_t)moved(cut); out.end = (uint32_t)end;
    out.last = next >= end;
    out.hi = out.last ? (uint32_t)end : (uint32_t)moved(next);
    return out;
}

// jpeg_fill for a lane: the reader ends at the piece's end `cut` first. When it gets there (its first zero bits), the real bits it has
// loaded since the entry's byte are the piece's (`budget`, -1 before), `stop` is where they ended, and, unless the interval ends there
// or a marker stands there, the zero bits leave again and the reader goes on to the interval's end.
__device__ __forceinline__ void jpeg_sync_fill(JpegBitReader& r, const uint8_t* cut, const uint8_t* end, int& loaded, int& budget, const uint8_t*& stop) {
    int before = r.n;
    jpeg_fill(r);
    loaded += r.n - before;
    if (budget < 0 && r.fake) {
        budget = loaded - r.fake;
        stop = r.p;
        if (r.p == cut && cut < end && r.fake < 64) {
            r.acc >>= r.fake; r.n -= r.fake; loaded -= r.fake; r.fake = 0; r.end = end;
            before = r.n;
            jpeg_fill(r);
            loaded += r.n - before;
        }
    }
}

struct JpegSyncRun { uint2 exit; uint32_t slots, dc0, dc1, dc2, flags; };

// One piece from `entry`. WRITE: `out` is the interval's first slot, `total` its slots, `first` the lane's first slot, predictor0…2 the DC
// values in front of it; run.flags collects SFX_JPEG_* bits.
template <bool WRITE>
__device__ __forceinline__ void jpeg_sync_decode(const JpegHuffmanLookup& h, const sfx_jpeg_frame& f, const JpegDecodeGeometry& g, const uint8_t* scan, const JpegSyncLane& lane,
                                                 uint2 entry, int16_t* out, unsigned long long total, unsigned long long first, uint32_t predictor0, uint32_t predictor1,
                                                 uint32_t predictor2, JpegSyncRun& run) {
    run.slots = 0u; run.dc0 = run.dc1 = run.dc2 = 0u; run.flags = 0u;
    if (!(entry.y & JPEG_SYNC_VALID)) {
        if (WRITE) { run.exit = entry; return; }                        // the lane in front met a real error (and has reported it)
        entry = make_uint2(lane.lo, JPEG_SYNC_VALID);                   // the rounds: the lane in front ran into nonsense; assume again
    }
    run.exit = entry;
    const uint32_t byte = entry.x;
    const int bit = (int)(entry.y & 255u);
    int b = (int)((entry.y >> 8) & 255u), k = (int)((entry.y >> 16) & 255u);
    if (byte < lane.lo || byte > lane.end || bit > 7 || b >= g.blocks || k > 63) { run.exit = make_uint2(0u, 0u); return; }
    if (byte >= lane.hi) return;                                        // entered beyond its own end: the state passes through
    const uint8_t* cut = scan + lane.hi;
    const uint8_t* end = scan + lane.end;
    const uint8_t* stop = cut;
    JpegBitReader reader{scan + byte, cut, 0ull, 0, 0};
    int loaded = 0, budget = -1;
    jpeg_sync_fill(reader, cut, end, loaded, budget, stop);
    jpeg_take(reader, bit);
    const int luma_blocks = g.components == 1 ? 1 : g.hs*g.vs;
    const int limit = 8*(int)(lane.hi - byte) + 8;                      // a symbol takes a bit at least
    unsigned long long slot = first;
    uint32_t flags = 0u;
    bool ended = false;
    auto zeros = [&](int count) {
        if (WRITE) for (int z = 0; z < count; z++) if (slot + (unsigned)z < total) out[slot + (unsigned)z] = 0;
        slot += (unsigned)count;
    };
    for (int step = 0; step < limit; step++) {
        jpeg_sync_fill(reader, cut, end, loaded, budget, stop);
        if (budget >= 0 && loaded - reader.n >= budget) { ended = true; break; }
        if (WRITE && slot >= total) { ended = true; break; }
        const int component = b < luma_blocks ? 0 : b - luma_blocks + 1;
        if (k == 0) {
            const int size = jpeg_symbol(reader, h, f.td[component] & 1);
            if (size < 0 || size > 15) { flags |= SFX_JPEG_BAD_CODE; break; }
            const uint32_t difference = (uint32_t)jpeg_extend(jpeg_take(reader, size), size);
            uint32_t& sum = component == 0 ? run.dc0 : (component == 1 ? run.dc1 : run.dc2);
            sum += difference;
            if (WRITE && slot < total) out[slot] = (int16_t)(int)((component == 0 ? predictor0 : (component == 1 ? predictor1 : predictor2)) + sum);
            slot++; k = 1;
        } else {
            const int code = jpeg_symbol(reader, h, 2 + (f.ta[component] & 1));
            if (code < 0) { flags |= SFX_JPEG_BAD_CODE; break; }
            const int zero_run = code >> 4, size = code & 15;
            if (size == 0) {
                if (zero_run != 15) { zeros(64 - k); k = 64; }          // EOB
                else {
                    if (k + 16 > 64) { flags |= SFX_JPEG_BAD_RUN; break; }
                    zeros(16); k += 16;
                }
            } else {
                if (k + zero_run > 63) { flags |= SFX_JPEG_BAD_RUN; break; }
                zeros(zero_run); k += zero_run;
                const int value = jpeg_extend(jpeg_take(reader, size), size);
                if (WRITE && slot < total) out[slot] = (int16_t)value;
                slot++; k++;
            }
        }
        if (k >= 64) { k = 0; b = b + 1 < g.blocks ? b + 1 : 0; }
        if (reader.n < reader.fake) { flags |= SFX_JPEG_OUT_OF_BITS; break; }
    }
    run.flags = flags;
    run.slots = (uint32_t)(slot - first);
    if (WRITE) return;
    if (!ended) { run.exit = make_uint2(0u, 0u); return; }
    const int past = loaded - reader.n - budget;                        // bits of the last symbol beyond the piece: at most 31
    const uint8_t* q = stop;
    for (int n = 0; n < (past >> 3) && n < 4; n++)
        if (q < end) q += (*q == 0xffu && q + 1 < end && q[1] == 0u) ? 2 : 1;
    if (q > end) q = end;
    run.exit = make_uint2((uint32_t)(q - scan), (uint32_t)(past & 7) | ((uint32_t)b << 8) | ((uint32_t)k << 16) | JPEG_SYNC_VALID);
}

__global__ void __launch_bounds__(JPEG_SYNC_LANES) k_jpeg_sync_rounds(const uint8_t* __restrict__ frame, JpegSyncScratch scratch, JpegDecodeGeometry g, uint32_t subsequence,
                                                                      int budget, int phase) {
    __shared__ JpegHuffmanLookup tables;
    __shared__ uint2 exits[JPEG_SYNC_LANES];
    const int t = threadIdx.x;
    const sfx_jpeg_frame& f = *reinterpret_cast<const sfx_jpeg_frame*>(frame);
    if (!jpeg_sync_sane(f, g, scratch, subsequence, (unsigned long long)gridDim.x*JPEG_SYNC_LANES)) return;      // (uniform; k_jpeg_sync_scan hands the frame to the fall-back)
    jpeg_build_lookup(tables, f, t, JPEG_SYNC_LANES);
    const unsigned long long lanes = jpeg_sync_lanes(f.scan_bytes, f.intervals, subsequence), index = (unsigned long long)blockIdx.x*JPEG_SYNC_LANES + t;
    const bool mine = index < lanes;
    const uint8_t* scan = frame + f.scan_offset;
    JpegSyncLane lane{JPEG_SYNC_IDLE, 0u, 0u, 0u, 0u, false};
    if (mine) lane = jpeg_sync_lane(frame, f, subsequence, index);
    const bool idle = (lane.flags & JPEG_SYNC_IDLE) != 0u, head = (lane.flags & JPEG_SYNC_HEAD) != 0u;
    uint2 entry = make_uint2(lane.lo, JPEG_SYNC_VALID);                 // bit 0, b = 0, k = 0: known for a head, assumed for the others
    JpegSyncRun run{make_uint2(0u, 0u), 0u, 0u, 0u, 0u, 0u};
    if (phase == 0) {
        if (!idle) jpeg_sync_decode<false>(tables, f, g, scan, lane, entry, nullptr, 0ull, 0ull, 0u, 0u, 0u, run);
    } else if (mine) {
        const JpegSyncRecord& r = scratch.records[index];
        entry = r.entry; run.exit = r.exit; run.slots = r.slots; run.dc0 = r.dc[0]; run.dc1 = r.dc[1]; run.dc2 = r.dc[2];
    }
    exits[t] = run.exit;
    uint32_t used = 0u;
    for (int round = 0; round < budget; round++) {
        __syncthreads();
        uint2 want = entry;
        if (!idle && !head) {
            if (t > 0) want = exits[t - 1];
            else if (phase == 1 && round == 0 && blockIdx.x > 0) want = scratch.handoff[blockIdx.x - 1];
        }
        const bool changed = want.x != entry.x || want.y != entry.y;
        if (!__syncthreads_or(changed ? 1 : 0)) break;
        used = (uint32_t)round + 1u;
        if (changed) {
            entry = want;
            jpeg_sync_decode<false>(tables, f, g, scan, lane, entry, nullptr, 0ull, 0ull, 0u, 0u, 0u, run);
        }
        exits[t] = run.exit;
    }
    if (mine) {
        JpegSyncRecord& r = scratch.records[index];
        r.entry = entry; r.exit = run.exit; r.slots = run.slots; r.dc[0] = run.dc0; r.dc[1] = run.dc1; r.dc[2] = run.dc2; r.flags = lane.flags;
    }
    if (phase == 0 && t == JPEG_SYNC_LANES - 1) scratch.handoff[blockIdx.x] = run.exit;
    if (t == 0) scratch.rounds[(size_t)phase*gridDim.x + blockIdx.x] = used;
}

// `workgroups`, `phases`: of the k_jpeg_sync_rounds launches in front
__global__ void __launch_bounds__(JPEG_SYNC_LANES) k_jpeg_sync_scan(const uint8_t* __restrict__ frame, JpegSyncScratch scratch, JpegDecodeGeometry g, uint32_t subsequence,
                                                                    uint32_t workgroups, int phases) {
    __shared__ unsigned long long carry_slots[JPEG_SYNC_LANES];
    __shared__ uint32_t carry_dc[3][JPEG_SYNC_LANES], closed[JPEG_SYNC_LANES], most[2];
    const int t = threadIdx.x;
    const sfx_jpeg_frame& f = *reinterpret_cast<const sfx_jpeg_frame*>(frame);
    if (!jpeg_sync_sane(f, g, scratch, subsequence, (unsigned long long)workgroups*JPEG_SYNC_LANES)) {
        if (t == 0) { scratch.control[0] = 1u; scratch.control[1] = 0u; scratch.control[2] = 0u; }
        return;
    }
    const unsigned long long lanes = jpeg_sync_lanes(f.scan_bytes, f.intervals, subsequence);
    const unsigned long long each = (lanes + JPEG_SYNC_LANES - 1ull)/JPEG_SYNC_LANES;
    const unsigned long long from = each*t < lanes ? each*t : lanes, to = from + each < lanes ? from + each : lanes;
    if (t < 2) most[t] = 0u;
    // 1. every thread's run of records: the sums behind its last head
    unsigned long long slots = 0ull;
    uint32_t dc0 = 0u, dc1 = 0u, dc2 = 0u, heads = 0u;
    for (unsigned long long n = from; n < to; n++) {
        const JpegSyncRecord& r = scratch.records[n];
        if (r.flags & JPEG_SYNC_IDLE) continue;
        if (r.flags & JPEG_SYNC_HEAD) { slots = 0ull; dc0 = dc1 = dc2 = 0u; heads = 1u; }
        slots += r.slots; dc0 += r.dc[0]; dc1 += r.dc[1]; dc2 += r.dc[2];
    }
    carry_slots[t] = slots; carry_dc[0][t] = dc0; carry_dc[1][t] = dc1; carry_dc[2][t] = dc2; closed[t] = heads;
    __syncthreads();
    // 2. what stands in front of every run: 256 terms, one thread
    if (t == 0) {
        slots = 0ull; dc0 = dc1 = dc2 = 0u;
        for (int n = 0; n < JPEG_SYNC_LANES; n++) {
            const unsigned long long s = carry_slots[n];
            const uint32_t a = carry_dc[0][n], b = carry_dc[1][n], c = carry_dc[2][n];
            carry_slots[n] = slots; carry_dc[0][n] = dc0; carry_dc[1][n] = dc1; carry_dc[2][n] = dc2;
            if (closed[n]) { slots = s; dc0 = a; dc1 = b; dc2 = c; } else { slots += s; dc0 += a; dc1 += b; dc2 += c; }
        }
    }
    for (uint32_t n = t; n < workgroups*(uint32_t)(phases > 2 ? 2 : phases); n += JPEG_SYNC_LANES) atomicMax(&most[n/workgroups], scratch.rounds[n]);
    __syncthreads();
    // 3. the exclusive sums into the records, and the fixed point's test
    slots = carry_slots[t]; dc0 = carry_dc[0][t]; dc1 = carry_dc[1][t]; dc2 = carry_dc[2][t];
    int open = 0;
    for (unsigned long long n = from; n < to; n++) {
        JpegSyncRecord& r = scratch.records[n];
        if (r.flags & JPEG_SYNC_IDLE) continue;
        if (r.flags & JPEG_SYNC_HEAD) { slots = 0ull; dc0 = dc1 = dc2 = 0u; }
        else if (n == 0ull) open = 1;
        else {
            const uint2 left = scratch.records[n - 1ull].exit;
            if (left.x != r.entry.x || left.y != r.entry.y) open = 1;
        }
        r.first[0] = (uint32_t)slots; r.first[1] = (uint32_t)(slots >> 32); r.predictor[0] = dc0; r.predictor[1] = dc1; r.predictor[2] = dc2;
        slots += r.slots; dc0 += r.dc[0]; dc1 += r.dc[1]; dc2 += r.dc[2];
    }
    open = __syncthreads_or(open);
    if (t == 0) { scratch.control[0] = open ? 1u : 0u; scratch.control[1] = most[0] + most[1]; scratch.control[2] = (uint32_t)lanes; }
}

__global__ void __launch_bounds__(JPEG_SYNC_LANES) k_jpeg_sync_write(const uint8_t* __restrict__ frame, int16_t* __restrict__ coefficients, uint32_t* __restrict__ status,
                                                                     JpegSyncScratch scratch, JpegDecodeGeometry g, uint32_t subsequence) {
    __shared__ JpegHuffmanLookup tables;
    const int t = threadIdx.x;
    if (scratch.control[0] != 0u) return;                               // (uniform) the fall-back's frame
    const sfx_jpeg_frame& f = *reinterpret_cast<const sfx_jpeg_frame*>(frame);
    if (!jpeg_sync_sane(f, g, scratch, subsequence, (unsigned long long)gridDim.x*JPEG_SYNC_LANES)) return;      // (control[0] is set then: not reached)
    jpeg_build_lookup(tables, f, t, JPEG_SYNC_LANES);
    const unsigned long long lanes = jpeg_sync_lanes(f.scan_bytes, f.intervals, subsequence), index = (unsigned long long)blockIdx.x*JPEG_SYNC_LANES + t;
    const uint8_t* scan = frame + f.scan_offset;
    const uint32_t scan_bytes = f.scan_bytes, intervals = f.intervals, restart = f.restart;
    uint32_t flags = 0u;
    if (index < intervals) {                                            // interval `index`: its marker, and whether it has bytes at all
        const uint32_t* offsets = reinterpret_cast<const uint32_t*>(frame + JPEG_FRAME_FIXED);
        const uint32_t interval = (uint32_t)index;
        const unsigned long long begin = offsets[interval], finish = interval + 1u < intervals ? (unsigned long long)offsets[interval + 1u] : (unsigned long long)scan_bytes + 2ull;
        flags = jpeg_interval_fault(scan, scan_bytes, interval, begin, finish);
        if (!flags && finish == begin + 2ull) flags = SFX_JPEG_OUT_OF_BITS;
    }
    if (index < lanes) {
        const JpegSyncLane lane = jpeg_sync_lane(frame, f, subsequence, index);
        if (!(lane.flags & JPEG_SYNC_IDLE)) {
            const JpegSyncRecord& r = scratch.records[index];
            const unsigned long long all = (unsigned long long)g.mcus_x*g.mcus_y, first_mcu = (unsigned long long)lane.interval*restart;
            const unsigned long long mcus = all - first_mcu < restart ? all - first_mcu : restart, total = mcus*g.blocks*64ull;
            const unsigned long long first = (unsigned long long)r.first[0] | ((unsigned long long)r.first[1] << 32);
            JpegSyncRun run;
            jpeg_sync_decode<true>(tables, f, g, scan, lane, r.entry, coefficients + (size_t)first_mcu*g.blocks*64, total, first, r.predictor[0], r.predictor[1], r.predictor[2], run);
            flags |= run.flags;
            if (lane.last && !run.flags && first + run.slots < total) flags |= SFX_JPEG_OUT_OF_BITS;     // the interval's lanes end short of its slots
        }
    }
    if (flags) atomicOr(status, flags);
}

// ---- 2. dequantisation and the inverse DCT → the components' planes --------------------------------------------------------------------
// 256 threads = four 8 x 8 blocks, a thread per term in both passes. The planes are padded to whole MCUs: luma mcus_x*hs*8 wide,
// chroma mcus_x*8. A frame whose status is bad is left alone (the texture keeps what it showed); the first such frame since the last
// question is noted in `first_bad` = {status, serial} (pinned host memory) for sfx_video_status.
__global__ void __launch_bounds__(256) k_jpeg_decode_planes(const sfx_jpeg_frame* __restrict__ frame, const int16_t* __restrict__ coefficients, uint8_t* __restrict__ planes,
                                                            const float* __restrict__ basis, const uint32_t* __restrict__ status, volatile uint32_t* first_bad, uint32_t serial,
                                                            JpegDecodeGeometry g) {
    __shared__ float dct[64];
    __shared__ float terms[4][64], rows[4][64];
    __shared__ __attribute__((aligned(8))) uint8_t samples[4][64];
    const int t = threadIdx.x, q = t >> 6, k = t & 63;
    const uint32_t bad = *status;
    if (bad) {
        if (first_bad && blockIdx.x == 0 && t == 0 && first_bad[0] == 0u) { first_bad[1] = serial; first_bad[0] = bad; }
        return;
    }
    const size_t total = (size_t)g.mcus_x*g.mcus_y*g.blocks, block = (size_t)blockIdx.x*4 + q;
    const bool live = block < total;
    const int luma_blocks = g.components == 1 ? 1 : g.hs*g.vs;
    const size_t mcu = block/g.blocks;
    const int b = (int)(block - mcu*g.blocks), component = b < luma_blocks ? 0 : b - luma_blocks + 1;
    if (t < 64) dct[t] = basis[t];
    int value = 0;
    if (live) value = (int)coefficients[block*64 + k]*(int)frame->quant[frame->tq[component] & 3][k];
    terms[q][JPEG_ZIGZAG.natural_of[k]] = (float)value;
    __syncthreads();
    const int hi = k >> 3, lo = k & 7;
    float acc = 0.0f;
#pragma unroll
    for (int u = 0; u < 8; u++) acc = fmaf(terms[q][hi*8 + u], dct[u*8 + lo], acc);       // row v = hi of the block's terms → sample column x = lo
    rows[q][k] = acc;
    __syncthreads();
    acc = 0.0f;
#pragma unroll
    for (int v = 0; v < 8; v++) acc = fmaf(rows[q][v*8 + lo], dct[v*8 + hi], acc);        // column x = lo → sample row y = hi
    const float rounded = floorf(acc + 128.0f + 0.5f);
    samples[q][k] = (uint8_t)(rounded < 0.0f ? 0.0f : (rounded > 255.0f ? 255.0f : rounded));
    __syncthreads();
    if (t < 32) {                                                       // a sample row of 8 bytes per thread
        const int group = t >> 3, row = t & 7;
        const size_t mine = (size_t)blockIdx.x*4 + group;
        if (mine < total) {
            const size_t at = mine/g.blocks;
            const int mb = (int)(mine - at*g.blocks), mc = mb < luma_blocks ? 0 : mb - luma_blocks + 1;
            const int mx = (int)(at % g.mcus_x), my = (int)(at/g.mcus_x);
            const int bx = mc == 0 && g.components == 3 ? mx*g.hs + mb % g.hs : mx, by = mc == 0 && g.components == 3 ? my*g.vs + mb/g.hs : my;
            const size_t pitch = (size_t)g.mcus_x*8*(mc == 0 && g.components == 3 ? g.hs : 1);
            *reinterpret_cast<uint2*>(planes + jpeg_plane_offset(g, mc) + ((size_t)by*8 + row)*pitch + (size_t)bx*8) = *reinterpret_cast<const uint2*>(&samples[group][row*8]);
        }
    }
}

// ---- 3. upsampling, colour, row flip → RGB8 -------------------------------------------------------------------------------------------
constexpr int JPEG_RUN = 16;                                        // pixels per lane

__device__ __forceinline__ int jpeg_clamp(int v, int last) { return v < 0 ? 0 : (v > last ? last : v); }       // into 0…last
__device__ __forceinline__ uint32_t jpeg_clip8(int v) { return (uint32_t)(v < 0 ? 0 : (v > 255 ? 255 : v)); }

// the upsampled chroma of the 16 pixels from x0 on row y (x0 a multiple of 16): the triangle filter of the header's definition
__device__ __forceinline__ void jpeg_chroma_run(const uint8_t* __restrict__ plane, int pitch, int cw, int ch, int hs, int vs, int x0, int y, int (&out)[JPEG_RUN]) {
    if (hs == 1) {
        const uint8_t* row = plane + (size_t)y*pitch;
#pragma unroll
        for (int i = 0; i < JPEG_RUN; i++) out[i] = row[jpeg_clamp(x0 + i, cw - 1)];
        return;
    }
    const int near = y/vs, far = jpeg_clamp(near + ((y & 1) ? 1 : -1), ch - 1);
    const uint8_t* a = plane + (size_t)near*pitch;
    const uint8_t* b = plane + (size_t)far*pitch;
    int s[JPEG_RUN/2 + 2];
#pragma unroll
    for (int i = 0; i < JPEG_RUN/2 + 2; i++) {
        const int j = jpeg_clamp(x0/2 - 1 + i, cw - 1);
        s[i] = vs == 2 ? 3*(int)a[j] + (int)b[j] : (int)a[j];
    }
#pragma unroll
    for (int i = 0; i < JPEG_RUN; i++) {
        const int sum = 3*s[i/2 + 1] + ((i & 1) ? s[i/2 + 2] : s[i/2]);
        out[i] = vs == 2 ? (sum + ((i & 1) ? 7 : 8)) >> 4 : (sum + ((i & 1) ? 2 : 1)) >> 2;
    }
}

__global__ void __launch_bounds__(256) k_jpeg_decode_pixels(const uint8_t* __restrict__ planes, uint8_t* __restrict__ dst, const uint32_t* __restrict__ status,
                                                            JpegDecodeGeometry g, int bottom_up) {
    if (*status) return;
    const int w = g.width, h = g.height, runs = (w + JPEG_RUN - 1)/JPEG_RUN;
    const long index = (long)blockIdx.x*256 + threadIdx.x;
    if (index >= (long)runs*h) return;
    const int y = (int)(index/runs), x0 = ((int)(index - (long)y*runs))*JPEG_RUN;
    const int n = (w - x0) < JPEG_RUN ? (w - x0) : JPEG_RUN;
    const bool colour = g.components == 3;
    const int luma_pitch = g.mcus_x*8*(colour ? g.hs : 1);
    const uint8_t* lp = planes + (size_t)y*luma_pitch + x0;
    int luma[JPEG_RUN], cb[JPEG_RUN], cr[JPEG_RUN];
    if (x0 + JPEG_RUN <= luma_pitch) {
        uint32_t l[4]; __builtin_memcpy(l, lp, 16);
#pragma unroll
        for (int i = 0; i < JPEG_RUN; i++) luma[i] = (int)((l[i >> 2] >> (8*(i & 3))) & 255u);
    } else {
#pragma unroll
        for (int i = 0; i < JPEG_RUN; i++) luma[i] = i < n ? (int)lp[i] : 0;
    }
    if (colour) {
        const int cw = (w + g.hs - 1)/g.hs, ch = (h + g.vs - 1)/g.vs, pitch = g.mcus_x*8;
        jpeg_chroma_run(planes + jpeg_plane_offset(g, 1), pitch, cw, ch, g.hs, g.vs, x0, y, cb);
        jpeg_chroma_run(planes + jpeg_plane_offset(g, 2), pitch, cw, ch, g.hs, g.vs, x0, y, cr);
    }
    uint32_t out[12];
#pragma unroll
    for (int k = 0; k < 12; k++) out[k] = 0u;
#pragma unroll
    for (int i = 0; i < JPEG_RUN; i++) {
        uint32_t rgb[3];
        if (colour) {
            const int d = cb[i] - 128, e = cr[i] - 128;
            rgb[0] = jpeg_clip8(luma[i] + ((91881*e + 32768) >> 16));
            rgb[1] = jpeg_clip8(luma[i] + ((-22554*d - 46802*e + 32768) >> 16));
            rgb[2] = jpeg_clip8(luma[i] + ((116130*d + 32768) >> 16));
        } else rgb[0] = rgb[1] = rgb[2] = (uint32_t)luma[i];
#pragma unroll
        for (int k = 0; k < 3; k++) { const int at = 3*i + k; out[at >> 2] |= rgb[k] << (8*(at & 3)); }
    }
    uint8_t* o = dst + ((size_t)(bottom_up ? h - 1 - y : y)*w + x0)*3;
    if (n == JPEG_RUN && w % JPEG_RUN == 0 && (reinterpret_cast<uintptr_t>(dst) & 15) == 0) {   // every row starts on a 16-byte boundary: three aligned stores
#pragma unroll
        for (int k = 0; k < 3; k++) reinterpret_cast<uint4*>(o)[k] = make_uint4(out[4*k], out[4*k + 1], out[4*k + 2], out[4*k + 3]);
    } else if (n == JPEG_RUN) {
        __builtin_memcpy(o, out, 48);
    } else {
#pragma unroll
        for (int i = 0; i < 3*JPEG_RUN; i++) if (i < 3*n) o[i] = (uint8_t)(out[i >> 2] >> (8*(i & 3)));
    }
}
inline long jpeg_pixel_lanes(int w, int h) { return (long)((w + JPEG_RUN - 1)/JPEG_RUN)*h; }

}  // namespace sf
