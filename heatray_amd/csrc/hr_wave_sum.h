// hr_wave_sum.h — waveSum, the one device helper the render stages (hr_wave.h) and the post-process kernels (hr_post_device.h) both use.
#pragma once
#include "hr_math.h" // HRD

namespace hr {

// the wave's sum of `v`, in every lane (the caller sees to it that it fits 32 bits)
HRD uint32_t waveSum(uint32_t v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o);
    return v;
}

} // namespace hr
