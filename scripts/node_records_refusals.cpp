// The argument checks of tm_nodes_drain, tm_nodes_sweep and tm_node_targets as a stand-alone program for a host sanitizer: every
// call below is refused before the first HIP call, so the program needs no GPU and follows none of the pointers it hands over.
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined \
//       scripts/node_records_refusals.cpp tetris_mcts_amd/csrc/node_records.hip -o node_records_refusals && ./node_records_refusals
// It prints the number of refusals it saw and exits 0, or names the first call that was not refused and exits 1.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include "../include/tetris_mcts_hip.h"

static int n_checked = 0, n_failed = 0;

static void expect(int got, int want, const char* what) {
    n_checked += 1;
    if (got != want) {
        n_failed += 1;
        std::fprintf(stderr, "%s: returned %d, expected %d\n", what, got, want);
    }
}

static tm_store store(void* p) {
    tm_store s;
    std::memset(&s, 0, sizeof s);
    s.n_games = 8; s.max_nodes = 64; s.kind = TM_KIND_VALUESIM; s.replay_cap = 5; s.online = 1; s.min_visits_to_store = 3;
    s.replay_obs = (uint32_t*)p; s.replay_stat = (float*)p; s.replay_count = (int32_t*)p;
    s.obs_stat = (uint32_t*)p; s.obs_key = (uint32_t*)p; s.gs = (int32_t*)p;
    return s;
}

static int sweep(tm_store* s, void* ring, int cap, int32_t* counters, int32_t* offsets, void* stream) {
    return tm_nodes_sweep(s, ring, cap, counters, offsets, stream);
}

int main() {
    alignas(16) static char buf[64];
    void* p = buf;
    void* odd = buf + 8;
    const int INVALID = 1;      // hipErrorInvalidValue
    int32_t* ip = (int32_t*)p;
    tm_store s = store(p);
    typedef int (*ring_call)(tm_store*, void*, int, int32_t*, int32_t*, void*);
    ring_call calls[2] = {tm_nodes_drain, sweep};
    const char* names[2] = {"tm_nodes_drain", "tm_nodes_sweep"};
    for (int k = 0; k < 2; ++k) {
        expect(calls[k](nullptr, p, 16, ip, ip, nullptr), INVALID, names[k]);
        expect(calls[k](&s, nullptr, 16, ip, ip, nullptr), INVALID, names[k]);
        expect(calls[k](&s, p, 16, nullptr, ip, nullptr), INVALID, names[k]);
        expect(calls[k](&s, p, 16, ip, nullptr, nullptr), INVALID, names[k]);
        expect(calls[k](&s, p, 0, ip, ip, nullptr), INVALID, names[k]);
        expect(calls[k](&s, p, -3, ip, ip, nullptr), INVALID, names[k]);
        expect(calls[k](&s, odd, 16, ip, ip, nullptr), INVALID, names[k]);
        tm_store d = store(p);
        d.kind = TM_KIND_DIST;
        expect(calls[k](&d, p, 16, ip, ip, nullptr), INVALID, names[k]);
        tm_store z = store(p);
        z.n_games = 0;
        expect(calls[k](&z, p, 16, ip, ip, nullptr), INVALID, names[k]);
    }
    for (int cap = -1; cap <= 0; ++cap) {
        tm_store c = store(p);
        c.replay_cap = cap;
        expect(tm_nodes_drain(&c, p, 16, ip, ip, nullptr), INVALID, "tm_nodes_drain replay_cap");
    }
    {
        tm_store a = store(p), b = store(p), c = store(p);
        a.replay_obs = nullptr; b.replay_stat = nullptr; c.replay_count = nullptr;
        expect(tm_nodes_drain(&a, p, 16, ip, ip, nullptr), INVALID, "tm_nodes_drain replay_obs");
        expect(tm_nodes_drain(&b, p, 16, ip, ip, nullptr), INVALID, "tm_nodes_drain replay_stat");
        expect(tm_nodes_drain(&c, p, 16, ip, ip, nullptr), INVALID, "tm_nodes_drain replay_count");
        tm_store d = store(p), e = store(p), f = store(p);
        d.obs_stat = nullptr; e.obs_key = nullptr; f.gs = nullptr;
        expect(tm_nodes_sweep(&d, p, 16, ip, ip, nullptr), INVALID, "tm_nodes_sweep obs_stat");
        expect(tm_nodes_sweep(&e, p, 16, ip, ip, nullptr), INVALID, "tm_nodes_sweep obs_key");
        expect(tm_nodes_sweep(&f, p, 16, ip, ip, nullptr), INVALID, "tm_nodes_sweep gs");
    }
    {
        tm_store a = store(p), b = store(p), c = store(p), d = store(p);      // the store's arrays are read as 16-byte pieces
        a.replay_obs = (uint32_t*)odd; b.replay_stat = (float*)odd; c.obs_stat = (uint32_t*)odd; d.obs_key = (uint32_t*)odd;
        expect(tm_nodes_drain(&a, p, 16, ip, ip, nullptr), INVALID, "tm_nodes_drain replay_obs alignment");
        expect(tm_nodes_drain(&b, p, 16, ip, ip, nullptr), INVALID, "tm_nodes_drain replay_stat alignment");
        expect(tm_nodes_sweep(&c, p, 16, ip, ip, nullptr), INVALID, "tm_nodes_sweep obs_stat alignment");
        expect(tm_nodes_sweep(&d, p, 16, ip, ip, nullptr), INVALID, "tm_nodes_sweep obs_key alignment");
    }
    uint32_t* up = (uint32_t*)p;
    float* fp = (float*)p;
    expect(tm_node_targets(nullptr, 10, 0, 0.001f, up, fp, fp, fp, ip, nullptr), INVALID, "tm_node_targets rows");
    expect(tm_node_targets(p, 10, 0, 0.001f, nullptr, fp, fp, fp, ip, nullptr), INVALID, "tm_node_targets obs");
    expect(tm_node_targets(p, 10, 0, 0.001f, up, nullptr, fp, fp, ip, nullptr), INVALID, "tm_node_targets value");
    expect(tm_node_targets(p, 10, 0, 0.001f, up, fp, nullptr, fp, ip, nullptr), INVALID, "tm_node_targets variance");
    expect(tm_node_targets(p, 10, 0, 0.001f, up, fp, fp, nullptr, ip, nullptr), INVALID, "tm_node_targets weight");
    expect(tm_node_targets(p, 10, 0, 0.001f, up, fp, fp, fp, nullptr, nullptr), INVALID, "tm_node_targets fault");
    expect(tm_node_targets(p, -1, 0, 0.001f, up, fp, fp, fp, ip, nullptr), INVALID, "tm_node_targets n_rows < 0");
    expect(tm_node_targets(p, 1 << 29, 0, 0.001f, up, fp, fp, fp, ip, nullptr), INVALID, "tm_node_targets n_rows 2^29");
    expect(tm_node_targets(p, 10, -1, 0.001f, up, fp, fp, fp, ip, nullptr), INVALID, "tm_node_targets weight_mode -1");
    expect(tm_node_targets(p, 10, 4, 0.001f, up, fp, fp, fp, ip, nullptr), INVALID, "tm_node_targets weight_mode 4");
    expect(tm_node_targets(odd, 10, 0, 0.001f, up, fp, fp, fp, ip, nullptr), INVALID, "tm_node_targets rows alignment");
    expect(tm_node_targets(p, 10, 0, 0.001f, (uint32_t*)(buf + 2), fp, fp, fp, ip, nullptr), INVALID, "tm_node_targets obs alignment");
    expect(tm_node_targets(p, 0, 0, 0.001f, up, fp, fp, fp, ip, nullptr), 0, "tm_node_targets n_rows == 0");
    std::printf("node_records refusals: %d checked, %d failed\n", n_checked, n_failed);
    return n_failed ? 1 : 0;
}
