// The exact three-way bf16 split of the split-precision ("bf16x3") backends and the activation rows built from it, shared by
// valuenet_x3.inc and distnet_x3.inc (each includes it inside its own namespace).  Numerics contracts: DESIGN.md sections 3.3 and 3.8.
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

// Activations in LDS: a row of X3_ROW bf16 per position = the hi, mid and lo planes of its 32 channels (channel innermost: a
// lane's eight consecutive k of one MFMA step are eight channels at one tap, one 16-byte read per plane) and 8 bf16 of
// padding (208-byte rows: a wave's 16-byte reads of consecutive positions fall on distinct bank groups).
constexpr int X3_ROW = 3 * 32 + 8;

struct Relu {
    static __device__ __forceinline__ float fwd(float v) { return v > 0.0f ? v : 0.0f; }
};
struct Leaky {      // LeakyReLU(0.01)
    static __device__ __forceinline__ float fwd(float v) { return v > 0.0f ? v : v * 0.01f; }
};

// Act of a 32 x 32 accumulator tile (lane: its position, channels (r & 3) + 8 (r >> 2) + 4 (l >> 5)) split into the three
// planes of the position's row: four runs of four consecutive channels, one 8-byte store per run and plane
template <typename Act>
__device__ __forceinline__ void store_planes(__bf16* row, const f32x16& acc, int half) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        bf16x4 h, m, l;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            __bf16 a, b, c;
            split3(Act::fwd(acc[4 * q + r]), a, b, c);
            h[r] = a;
            m[r] = b;
            l[r] = c;
        }
        __bf16* dst = row + 8 * q + 4 * half;
        *reinterpret_cast<bf16x4*>(dst) = h;
        *reinterpret_cast<bf16x4*>(dst + 32) = m;
        *reinterpret_cast<bf16x4*>(dst + 64) = l;
    }
}
