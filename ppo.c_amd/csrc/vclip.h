// vclip.h — one row of the value head (MSE, optionally with PPO2 value-loss clipping), written once for
// every form of the head: kernels.hip mse_kernel and value_head_kernel, out_head.hip HEAD == 0 (fp32 and
// bf16 storage) and the head carried by the x3 grad_W launch (gemm_x3.hip X3Args vh_*).
//
// ppo_ext.h ppo_set_value_clip states the semantics.  All arithmetic is fp32 in the order written here
// (the kernels are built with -ffp-contract=off); tests/vclip_ref.py mirrors it operation for operation.
#pragma once
#include <hip/hip_runtime.h>

#include "ppo_hip.h"

namespace ppo {

// Row i of a minibatch of m rows (mf = (float)m): y the network's value, t the target.  Returns the row's
// loss term l (the head sums l and divides by m) and sets g = ∂loss/∂y; clipped += 1 when the clipped term
// was taken.  vc.v_old == nullptr (off): l = (t − y)², g = 2(y − t)/m — the arithmetic of loss.cu:5-23, and
// the same for every row inside the clip range while it is on (an inside row never depends on whether
// v_old + (y − v_old) rounds back to y; a NaN d counts as inside and propagates as with clipping off).
__device__ __forceinline__ float value_head_row(float y, float t, float mf, const PhipVClip& vc, int i, float& g,
                                                int& clipped) {
    const float du = t - y;
    float l = du * du;
    g = 2 * (y - t) / mf;
    if (vc.v_old) {
        const float vo = vc.v_old[vc.rows ? vc.rows[i] : i];
        const float d = y - vo;
        if (fabsf(d) > vc.eps) {
            const float yc = vo + copysignf(vc.eps, d);
            const float dc = t - yc;
            const float lc = dc * dc;
            if (!(l >= lc)) {            // max() picks the clipped term (ties stay unclipped): its gradient is zero
                l = lc;
                g = 0.f;
                clipped += 1;
            }
        }
    }
    return l;
}

// += the head's two exact counters (clipped rows, rows), one 64-bit integer atomic each
__device__ __forceinline__ void value_clip_count(const PhipVClip& vc, unsigned long long clipped,
                                                 unsigned long long rows) {
    if (clipped) atomicAdd(vc.counts + 0, clipped);
    if (rows) atomicAdd(vc.counts + 1, rows);
}

}  // namespace ppo
