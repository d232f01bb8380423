// deep2_roles.h -- which of k_deep2's four wave bodies a wave of a workgroup enters (kernels_deep2.h).
// Plain C++: the kernel includes it for the device, the host compiler builds it for the test that runs every input
// (tests/test_deep2_roles_cpu.py).
//
// A workgroup is four waves: 0 front-down, 1 front-up, 2 back-down, 3 back-up.  A front wave issues four stage bodies and the gather
// per row, a back wave three and the stores; a CU holds two workgroups, every SIMD two waves, and the launch is bound by what a SIMD
// has to issue.  So a SIMD should hold a front wave of one workgroup and a back wave of the other -- which the role can only
// see to if it follows the SIMD the wave really runs on, not the wave's number in the workgroup: the dispatcher does not put wave w
// of every workgroup on SIMD w (profiles/deep2_priority_ab.txt, section 1).
//
// Every wave of a workgroup calls the function with the SAME four SIMD ids (published through LDS behind a barrier) and the same
// flip, and takes its own entry of role[]: the four waves cannot disagree, and role[] is a permutation of 0..3 for every input
// whatever the hardware reports -- two waves in one body would race on the LDS windows.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DEEP2_ROLES_FN __host__ __device__ inline
#else
#define DEEP2_ROLES_FN inline
#endif

// today's static rule, and the fall-back: roles by the wave's number, two waves on under flip
DEEP2_ROLES_FN int deep2_static_role(int w, int flip) { return (w + 2 * flip) & 3; }

// simd[w]: the SIMD id wave w of the workgroup reports; flip: 0 or 1, the same for all four waves
// role[w]: 0 front-down, 1 front-up, 2 back-down, 3 back-up -- ALWAYS a permutation of 0..3
// simd[] a permutation of 0..3: the role follows the SIMD -- flip 0: SIMDs 0, 1 hold the front waves (down, up), SIMDs 2, 3 the back
// waves; flip 1: the other way round, so that two workgroups of opposite flip put a front and a back wave on every SIMD of their CU.
// Any other input (two waves on one SIMD, a number out of range): the static rule.
DEEP2_ROLES_FN void deep2_assign_roles(const int simd[4], int flip, int role[4])
{
    flip &= 1;
    unsigned seen = 0;
    for (int w = 0; w < 4; ++w)
        if (simd[w] >= 0 && simd[w] < 4) seen |= 1u << simd[w];
    const bool by_simd = seen == 15u;                   // four ids in range that cover 0..3: a permutation
    for (int w = 0; w < 4; ++w) role[w] = by_simd ? ((simd[w] + 2 * flip) & 3) : deep2_static_role(w, flip);
}
