// piano_kernels.hpp — k_piano_frame: one frame of ShaderPiano.update() (shaderflow_amd/piano/module.py, the host mirror of the
// reference's piano/module.py:185-277) on the device. The score lives in HBM as structure-of-arrays grouped by pitch (CSR `first`,
// insertion order inside a pitch; start and end in float64, because every comparison of update() is made in float64 against the
// float64 clock), plus, per pitch, the same notes ordered by (whole second of their start, insertion index): `sorted`.
//
// One block per pitch writes that pitch's whole row of iPianoRoll (256 slots x RGBA32F = 4 KB, as coalesced 16-byte stores — no memset,
// no atomics: the block owns the row), its texel of iPianoChan, and steps its key of the key-press DynamicNumber into iPianoKeys.
//
// The reference visits the candidates of a pitch by (first whole-second bucket shared with the window, insertion index): first every
// note that has begun before the window's first second ends, in insertion order; then the later ones by starting second. That is two
// streaming passes — the CSR range as it is, then `sorted` — in which a note's slot is the number of visible candidates in front of it:
// a ballot and a population count per wave, the waves' totals through LDS. Nothing is serial in the number of notes, and a pitch with
// thousands of notes only takes more 256-note chunks. The second pass starts at the first later note (a binary search in `sorted`) and
// stops behind the window's last second, so it reads the window only; the first pass reads the pitch's whole list.
#pragma once

#include "dynamics_step.hpp"

namespace sf {

constexpr int PIANO_KEYS = 128;          // MAX_NOTE
constexpr int PIANO_SLOTS = 256;         // MAX_ROLLING
constexpr int PIANO_THREADS = 256;
constexpr int PIANO_STATE = 5;           // arrays of PIANO_KEYS floats in the state: value, derivative, previous, acceleration, target

struct PianoScore {
    const int* first;                    // [PIANO_KEYS + 1] CSR offsets
    const int* sorted;                   // [count] per pitch: indices into the arrays below, by (trunc(start), insertion index)
    const double* start; const double* end;
    const float* channel; const float* velocity;
};
struct PianoWindow { double time, visible_before, window_end, release_before_end; };

// the later of two (slot, value) pairs; slot -1: none
__device__ __forceinline__ void piano_later(int& slot, float& value, int other_slot, float other_value) {
    if (other_slot > slot) { slot = other_slot; value = other_value; }
}

__global__ __launch_bounds__(PIANO_THREADS) void k_piano_frame(PianoScore score, PianoWindow w, DynCoeffF32 c, int previous_is_target,
                                                               float* __restrict__ state, float* __restrict__ keys,
                                                               float* __restrict__ chan, float4* __restrict__ roll) {
    constexpr int WAVES = PIANO_THREADS/64;
    __shared__ float4 row[PIANO_SLOTS];
    __shared__ int wave_total[WAVES];
    __shared__ int last_slot[2][WAVES];
    __shared__ float last_value[2][WAVES];
    const int pitch = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    static_assert(PIANO_THREADS == PIANO_SLOTS, "one thread per slot of the row");
    row[threadIdx.x] = float4{0.0f, 0.0f, 0.0f, 0.0f};
    const int begin = score.first[pitch], end = score.first[pitch + 1];
    const double low = trunc(w.time), high = trunc(w.window_end);                 // int(time), int(time + lookup_time)
    int taken = 0;                                                                // visible candidates in front of this chunk
    int playing_slot = -1, pressed_slot = -1; float playing_channel = -1.0f, pressed_velocity = 0.0f;
    __syncthreads();
    // pass 1 starts at the first note of `sorted` that begins after the window's first second: the notes in front of it were pass 0's.
    // Every thread runs the same search on the same addresses, so the bound is uniform without a barrier.
    int later = begin;
    for (int above = end; later < above; ) {
        const int middle = (later + above) >> 1;
        if (trunc(score.start[score.sorted[middle]]) > low) above = middle; else later = middle + 1;
    }
    for (int pass = 0; pass < 2; pass++) {
        for (int at = pass ? later : begin; at < end; at += PIANO_THREADS) {
            // pass 1 walks the notes by starting second: nothing behind a note that starts after the window's last second is a candidate
            if (pass == 1 && trunc(score.start[score.sorted[at]]) > high) break;
            const int i = at + (int)threadIdx.x;
            bool visible = false;
            double s = 0.0, e = 0.0; int n = 0;
            if (i < end) {
                n = pass ? score.sorted[i] : i;
                s = score.start[n]; e = score.end[n];
                const double bucket = trunc(s);
                const bool candidate = (bucket <= high) && (trunc(e) >= low) && !(s > w.window_end) && (pass ? bucket > low : !(bucket > low));
                visible = candidate && (s < w.visible_before);
            }
            const unsigned long long mask = __ballot(visible);
            if (lane == 0) wave_total[wave] = __popcll(mask);
            __syncthreads();
            int slot = taken + __popcll(mask & ((1ull << lane) - 1ull)), total = 0;
#pragma unroll
            for (int k = 0; k < WAVES; k++) { if (k < wave) slot += wave_total[k]; total += wave_total[k]; }
            taken += total;
            if (visible) {
                const float channel = score.channel[n], velocity = score.velocity[n];
                if (slot < PIANO_SLOTS) row[slot] = float4{(float)s, (float)e, channel, velocity};
                // (a candidate whose slot was dropped still decides the key: module.py:185-188 index the visible ones, not the kept ones)
                const bool playing = (s <= w.time) && (w.time <= e);
                const bool pressed = playing && ((w.time < (e - w.release_before_end)) || ((e - s) < w.release_before_end));
                if (playing) piano_later(playing_slot, playing_channel, slot, channel);
                if (pressed) piano_later(pressed_slot, pressed_velocity, slot, velocity);
            }
            __syncthreads();                                                      // wave_total is written again by the next chunk
        }
    }
    // the last playing and the last pressed candidate of the pitch: a repeated index of numpy's assignment keeps its last value
    for (int m = 32; m >= 1; m >>= 1) {
        piano_later(playing_slot, playing_channel, __shfl_xor(playing_slot, m), __shfl_xor(playing_channel, m));
        piano_later(pressed_slot, pressed_velocity, __shfl_xor(pressed_slot, m), __shfl_xor(pressed_velocity, m));
    }
    if (lane == 0) {
        last_slot[0][wave] = playing_slot; last_value[0][wave] = playing_channel;
        last_slot[1][wave] = pressed_slot; last_value[1][wave] = pressed_velocity;
    }
    __syncthreads();                                                              // (also: every slot of `row` is written)
    roll[(long)pitch*PIANO_SLOTS + threadIdx.x] = row[threadIdx.x];
    if (threadIdx.x == 0) {
        for (int k = 1; k < WAVES; k++) {
            piano_later(playing_slot, playing_channel, last_slot[0][k], last_value[0][k]);
            piano_later(pressed_slot, pressed_velocity, last_slot[1][k], last_value[1][k]);
        }
        chan[pitch] = playing_slot >= 0 ? playing_channel : -1.0f;
        const float target = pressed_slot >= 0 ? pressed_velocity : 0.0f;
        float value = state[pitch], deriv = state[PIANO_KEYS + pitch], prev = state[2*PIANO_KEYS + pitch];
        // DynamicNumber.next leaves `previous` the same array object as `target` (reference dynamics.py:229), which update() then refills in
        // place: from the second step on, `previous` is the target of THIS frame
        if (previous_is_target) prev = target;
        if (c.dt != 0.0f) {                                                       // reference dynamics.py:210-211; precision == 0: no early-out
            state[3*PIANO_KEYS + pitch] = dynamics_step_f32(value, deriv, prev, target, c);
            state[pitch] = value; state[PIANO_KEYS + pitch] = deriv;
        }
        state[2*PIANO_KEYS + pitch] = prev;
        state[4*PIANO_KEYS + pitch] = target;
        keys[pitch] = value;
    }
}

}  // namespace sf
