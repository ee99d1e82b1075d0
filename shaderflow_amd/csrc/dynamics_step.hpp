// dynamics_step.hpp — one float32 step of DynamicNumber.next (reference dynamics.py:228-247), shared by the kernels that run the recurrence on the
// device: k_dynamics_scan (audio_kernels.hpp, the spectrogram bins of a batch) and k_piano_frame (piano_kernels.hpp, the 128 keys of a
// frame). The python scalars dt, k1, k2, k3 come from the host already rounded to float32, the way numpy rounds them for a float32
// array (NEP 50). One operation per line of the reference, in its order, none of them fused (the library is built with
// -ffp-contract=off): tests/golden/dynamics.npz pins the bits.
#pragma once

#include <hip/hip_runtime.h>

namespace sf {

struct DynCoeffF32 { float dt, k1, k2, k3; };

// Steps (value, derivative, previous) towards `target`; returns the acceleration the host object keeps. The caller has dealt with
// dt == 0 (reference dynamics.py:210-211) and with the early-out (:222-225).
__device__ __forceinline__ float dynamics_step_f32(float& value, float& deriv, float& prev, float target, const DynCoeffF32& c) {
    const float velocity = (target - prev)/c.dt;
    prev = target;
    value = value + (deriv*c.dt);
    const float accel = (((target + (c.k3*velocity)) - value) - (c.k1*deriv))/c.k2;
    deriv = deriv + (accel*c.dt);
    return accel;
}

}  // namespace sf
