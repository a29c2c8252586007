// What the two leaf evaluators (valuenet.hip, distnet.hip) share: the accumulator types of the fp32 matrix cores, the exponential
// of their numerics contracts and the wave-level LDS fence (each file includes it inside its own namespace, as bf16x3.h), and the
// host helper that raises a kernel's dynamic LDS limit once a process.
#pragma once
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

__device__ inline double tm_exp(double x) {
    if (x > 700.0) x = 700.0;
    if (x < -700.0) x = -700.0;
    const double inv_ln2 = 1.4426950408889634074, ln2_hi = 6.93147180369123816490e-01,
                 ln2_lo = 1.90821492927058770002e-10;
    double n = rint(x * inv_ln2);
    double r = fma(-n, ln2_hi, x);
    r = fma(-n, ln2_lo, r);
    double p = 1.0 / 6227020800.0;
    p = fma(p, r, 1.0 / 479001600.0);
    p = fma(p, r, 1.0 / 39916800.0);
    p = fma(p, r, 1.0 / 3628800.0);
    p = fma(p, r, 1.0 / 362880.0);
    p = fma(p, r, 1.0 / 40320.0);
    p = fma(p, r, 1.0 / 5040.0);
    p = fma(p, r, 1.0 / 720.0);
    p = fma(p, r, 1.0 / 120.0);
    p = fma(p, r, 1.0 / 24.0);
    p = fma(p, r, 1.0 / 6.0);
    p = fma(p, r, 0.5);
    p = fma(p, r, 1.0);
    p = fma(p, r, 1.0);
    long long bits = __double_as_longlong(p);
    bits += ((long long)n) << 52;
    return __longlong_as_double(bits);
}

__device__ __forceinline__ void lds_fence() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// hipFuncSetAttribute(MaxDynamicSharedMemorySize) for KERNEL, once a process; every call returns that one call's error
template <auto KERNEL>
static int max_dynamic_lds(int bytes) {
    static std::once_flag once;
    static int err = 0;
    std::call_once(once, [&] {
        err = (int)hipFuncSetAttribute(reinterpret_cast<const void*>(KERNEL), hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    });
    return err;
}
