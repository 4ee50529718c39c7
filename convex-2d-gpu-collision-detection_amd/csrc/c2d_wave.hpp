// c2d_wave.hpp — the small device helpers that several kernel files need and that must mean the same thing in each of them:
// the 16-byte float vector, the wave-wide u32 maximum and u64 minimum, the same-wave LDS hand-over and the register launder.
#pragma once

#include "c2d_math.hpp"

namespace c2d {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// the largest v of the wave's 64 lanes, wave-uniform (in an SGPR)
C2D_DEV uint32_t wave_max_u32(uint32_t v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const uint32_t o = (uint32_t)__shfl_xor((int)v, off, 64);
        v = o > v ? o : v;
    }
    return (uint32_t)__builtin_amdgcn_readfirstlane((int)v);
}

// the smallest v of the wave's 64 lanes, in lane 0 (the other lanes hold partial minima): the best key of a listed query
C2D_DEV unsigned long long wave_min_u64(unsigned long long v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long o = __shfl_down(v, off, 64);
        v = o < v ? o : v;
    }
    return v;
}

// LDS written by some lanes of a wave and read by others of the SAME wave (or read, then rewritten): a wave's LDS instructions
// execute in order, so only the compiler has to be kept from moving them across this point.  The fence pair does that and emits
// no instruction.
C2D_DEV void wave_lds_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// A value through an empty asm: the compiler can no longer tell that it is the value it already has projections of.  The
// certified rectangle paths pass the inputs of their eight-axis fall-back through it, or every projection of the fast path is
// kept alive for reuse there (172 spilled dwords in the headline kernel).  The tag chooses at compile time, so that one lambda
// can build a pair either way.
struct Plain {};
struct Laundered {};
C2D_DEV float launder(float x, Plain) { return x; }
C2D_DEV float launder(float x, Laundered)
{
    asm volatile("" : "+v"(x));
    return x;
}

}  // namespace c2d
