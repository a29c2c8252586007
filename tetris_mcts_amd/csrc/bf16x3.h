// The exact three-way bf16 split of the split-precision ("bf16x3") backends, shared by valuenet_x3.inc and distnet_x3.inc
// (each includes it inside its own namespace).  Numerics contracts: DESIGN.md sections 3.3 and 3.8.
#pragma once
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));

// x = hi + mid + lo (+ a remainder below 2^-24 |x|), each plane a bf16 value rounded to nearest even: hi = bf16(x),
// mid = bf16(x - hi), lo = bf16(x - hi - mid); both differences are exact in fp32
__device__ __forceinline__ void split3(float x, __bf16& hi, __bf16& mid, __bf16& lo) {
    hi = (__bf16)x;
    const float r1 = x - (float)hi;
    mid = (__bf16)r1;
    lo = (__bf16)(r1 - (float)mid);
}
