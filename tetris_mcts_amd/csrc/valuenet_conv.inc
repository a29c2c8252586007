// The convolution kernel of the value net (included by valuenet.hip): render + conv1 + conv2 + conv3 of one state per wave.
__global__ __launch_bounds__(256, CONV_WAVES_PER_SIMD) void k_vn_conv(const float* __restrict__ P, const float* __restrict__ prep,
                                                    const int8_t* __restrict__ states, const uint32_t* __restrict__ obs_key,
                                                    ReqList rq, int max_nodes,
                                                    int n, float* __restrict__ a3out, int a3stride,
                                                    int32_t* __restrict__ tile_cnt, int tile_cnt_stride) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    // k_vn_fc1's arrival counters (one per tile of 32 or 64 states: the pad word of every 32nd scratch row covers both tilings)
    // start every evaluation at zero whatever the scratch held - uninitialised memory, another kernel's leftovers, the count
    // of a launch that was aborted between two arrivals.  Ordered before fc1 by the kernel boundary.
    if (blockIdx.x == 0)
        for (int t = threadIdx.x; t < (n + 31) / 32; t += 256) tile_cnt[(size_t)t * tile_cnt_stride] = 0;
    // (one wave's work, state after state: valuenet_conv_body.inc, the text k_vn_conv_fc1 runs as its first phase)
#define CONV_WAVES 4
#define CONV_A3_STORE(ptr, val) (*(ptr) = (val))
#define CONV_STATE_DONE() do { } while (0)
#include "valuenet_conv_body.inc"
#undef CONV_WAVES
#undef CONV_A3_STORE
#undef CONV_STATE_DONE
}
