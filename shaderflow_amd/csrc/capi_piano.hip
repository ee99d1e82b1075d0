// capi_piano.hip — the C-ABI's piano-roll part (include/shaderflow_hip.h: sfx_piano_*): the score of a ShaderPiano in device memory, the
// state of its key-press DynamicNumber, and the launch of k_piano_frame (piano_kernels.hpp) that makes one frame's iPianoKeys, iPianoChan
// and iPianoRoll inside the scene's own textures. capi.hip's run_sequence launches the same frame in front of every frame's draws
// (piano_launch_frame, host_state.hpp).

#include "host_state.hpp"
#include "piano_kernels.hpp"

#include <cmath>

using namespace sf;

struct Piano : Object {
    Context* ctx;
    int count = 0;
    sfx_piano_params params;
    void* block = nullptr;                // one allocation: first | sorted | start | end | channel | velocity | state
    PianoScore score;
    float* state = nullptr;               // [PIANO_STATE][PIANO_KEYS]
    sfx_handle keys = 0, chan = 0, roll = 0;
};

static Texture* piano_texture(sfx_handle h, Context* c, int width, int height, int components) {
    Texture* t = get<Texture>(h, MAGIC_TEX);
    if (!t || t->ctx != c || t->dtype != SFX_F32 || t->width != width || t->height != height || t->components != components || !t->data) return nullptr;
    if (t->nbytes < (size_t)width*height*components*sizeof(float)) return nullptr;
    return t;
}

static size_t align16(size_t n) { return (n + 15) & ~(size_t)15; }

extern "C" int sfx_piano_create(sfx_handle hc, const int32_t* first, const int32_t* sorted, const double* start, const double* end,
                                const float* channel, const float* velocity, int count, const sfx_piano_params* params,
                                sfx_handle keys, sfx_handle chan, sfx_handle roll, const float* state, sfx_handle* out) {
    CTX_OR_FAIL(c, hc);
    if (!first || !params || !out || count < 0 || (count > 0 && (!sorted || !start || !end || !channel || !velocity)))
        return fail(SFX_E_INVALID, "piano: null score arrays, parameters or output");
    // the CSR table and the start-sorted index decide what the kernel reads: checked here, once
    if (first[0] != 0 || first[PIANO_KEYS] != count) return fail(SFX_E_INVALID, "piano: the pitch table does not cover the %d notes", count);
    for (int p = 0; p < PIANO_KEYS; p++) {
        if (first[p + 1] < first[p]) return fail(SFX_E_INVALID, "piano: the pitch table decreases at pitch %d", p);
        double before = -INFINITY;
        for (int k = first[p]; k < first[p + 1]; k++) {
            if (sorted[k] < first[p] || sorted[k] >= first[p + 1]) return fail(SFX_E_INVALID, "piano: start-sorted index %d leaves pitch %d", k, p);
            if (!std::isfinite(start[k]) || !std::isfinite(end[k])) return fail(SFX_E_INVALID, "piano: note %d has no finite start and end", k);
            const double second = std::trunc(start[sorted[k]]);
            if (second < before) return fail(SFX_E_INVALID, "piano: the start-sorted index of pitch %d is not sorted", p);
            before = second;
        }
    }
    if (!piano_texture(keys, c, PIANO_KEYS, 1, 1) || !piano_texture(chan, c, PIANO_KEYS, 1, 1) || !piano_texture(roll, c, PIANO_SLOTS, PIANO_KEYS, 4))
        return fail(SFX_E_INVALID, "piano: iPianoKeys / iPianoChan must be 128 x 1 R32F and iPianoRoll 256 x 128 RGBA32F textures of this context");
    USE_DEVICE(c);
    const size_t n = (size_t)count;
    const size_t at_first = 0, at_sorted = at_first + align16(sizeof(int)*(PIANO_KEYS + 1)), at_start = at_sorted + align16(sizeof(int)*n),
                 at_end = at_start + align16(sizeof(double)*n), at_channel = at_end + align16(sizeof(double)*n),
                 at_velocity = at_channel + align16(sizeof(float)*n), at_state = at_velocity + align16(sizeof(float)*n),
                 total = at_state + sizeof(float)*PIANO_STATE*PIANO_KEYS;
    Piano* p = new Piano();
    p->magic = MAGIC_PIANO; p->ctx = c; p->count = count; p->params = *params; p->keys = keys; p->chan = chan; p->roll = roll;
    if (hipMalloc(&p->block, total) != hipSuccess) { delete p; (void)hipGetLastError(); return fail(SFX_E_HIP, "piano: out of device memory (%zu bytes)", total); }
    char* base = (char*)p->block;
    p->score = PianoScore{(const int*)(base + at_first), (const int*)(base + at_sorted), (const double*)(base + at_start), (const double*)(base + at_end),
                          (const float*)(base + at_channel), (const float*)(base + at_velocity)};
    p->state = (float*)(base + at_state);
    bool ok = hipMemcpy(base + at_first, first, sizeof(int)*(PIANO_KEYS + 1), hipMemcpyHostToDevice) == hipSuccess;
    if (n) {
        ok = ok && hipMemcpy(base + at_sorted, sorted, sizeof(int)*n, hipMemcpyHostToDevice) == hipSuccess
                && hipMemcpy(base + at_start, start, sizeof(double)*n, hipMemcpyHostToDevice) == hipSuccess
                && hipMemcpy(base + at_end, end, sizeof(double)*n, hipMemcpyHostToDevice) == hipSuccess
                && hipMemcpy(base + at_channel, channel, sizeof(float)*n, hipMemcpyHostToDevice) == hipSuccess
                && hipMemcpy(base + at_velocity, velocity, sizeof(float)*n, hipMemcpyHostToDevice) == hipSuccess;
    }
    ok = ok && (state ? hipMemcpy(p->state, state, sizeof(float)*PIANO_STATE*PIANO_KEYS, hipMemcpyHostToDevice)
                      : hipMemset(p->state, 0, sizeof(float)*PIANO_STATE*PIANO_KEYS)) == hipSuccess;
    if (!ok) { hipFree(p->block); delete p; (void)hipGetLastError(); return fail(SFX_E_HIP, "piano: uploading the score failed"); }
    *out = handle_of(p);
    return SFX_OK;
}

// One frame on the context's render stream, in stream order with the draws behind it
int piano_launch_frame(sfx_handle h, Context* c, double scene_time, const sfx_dyn_coeff_f32& coeff, int previous_is_target) {
    Piano* p = get<Piano>(h, MAGIC_PIANO);
    if (!p) return fail(SFX_E_INVALID, "invalid piano handle");
    if (c && p->ctx != c) return fail(SFX_E_INVALID, "piano: the handle belongs to another context");
    // (the scene may have re-made a texture since sfx_piano_create: a stale handle is an error, not a write into freed memory)
    Texture *keys = piano_texture(p->keys, p->ctx, PIANO_KEYS, 1, 1), *chan = piano_texture(p->chan, p->ctx, PIANO_KEYS, 1, 1),
            *roll = piano_texture(p->roll, p->ctx, PIANO_SLOTS, PIANO_KEYS, 4);
    if (!keys || !chan || !roll) return fail(SFX_E_INVALID, "piano: a texture of the module was released or re-made after sfx_piano_create");
    const double time = scene_time + p->params.time_offset;                       // module.py: time = scene.time + time_offset
    const double lookup_time = p->params.roll_time + p->params.lookahead;
    const PianoWindow w{time, time + p->params.roll_time, time + lookup_time, p->params.release_before_end};
    const DynCoeffF32 k{coeff.dt, coeff.k1, coeff.k2, coeff.k3};
    hipLaunchKernelGGL(k_piano_frame, dim3(PIANO_KEYS), dim3(PIANO_THREADS), 0, p->ctx->stream, p->score, w, k, previous_is_target ? 1 : 0,
                       p->state, (float*)keys->data, (float*)chan->data, (float4*)roll->data);
    return launch_status();
}

extern "C" int sfx_piano_step(sfx_handle h, double scene_time, const sfx_dyn_coeff_f32* coeff, int previous_is_target) {
    Piano* p = get<Piano>(h, MAGIC_PIANO);
    if (!p || !coeff) return fail(SFX_E_INVALID, "invalid piano handle or null coefficients");
    USE_DEVICE(p->ctx);
    return piano_launch_frame(h, p->ctx, scene_time, *coeff, previous_is_target);
}

extern "C" int sfx_piano_state_read(sfx_handle h, float* state) {
    Piano* p = get<Piano>(h, MAGIC_PIANO);
    if (!p || !state) return fail(SFX_E_INVALID, "invalid piano handle or null output");
    USE_DEVICE(p->ctx);
    HIP_TRY(hipMemcpyAsync(state, p->state, sizeof(float)*PIANO_STATE*PIANO_KEYS, hipMemcpyDeviceToHost, p->ctx->stream));
    HIP_TRY(hipStreamSynchronize(p->ctx->stream));
    return SFX_OK;
}

extern "C" int sfx_piano_destroy(sfx_handle h) {
    Piano* p = get<Piano>(h, MAGIC_PIANO);
    if (!p) return fail(SFX_E_INVALID, "invalid piano handle");
    hipSetDevice(p->ctx->device);
    hipStreamSynchronize(p->ctx->stream);
    hipFree(p->block);
    p->magic = 0;
    delete p;
    return SFX_OK;
}
