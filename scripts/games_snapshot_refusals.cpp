// The argument checks of tm_env_check, tm_env_save, tm_env_load and tm_episode_resume as a stand-alone program for a host sanitizer:
// every call below is refused before the first HIP call, so the program needs no GPU and follows none of the pointers it hands over.
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined \
//       scripts/games_snapshot_refusals.cpp tetris_mcts_amd/csrc/games_snapshot.hip -o games_snapshot_refusals && ./games_snapshot_refusals
// It prints the number of refusals it saw and exits 0, or names the first call that was not refused and exits 1.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include "../include/tetris_mcts_hip.h"

static int n_checked = 0, n_failed = 0;

static void expect(int got, const char* what) {
    n_checked += 1;
    if (got != 1) {      // hipErrorInvalidValue
        n_failed += 1;
        std::fprintf(stderr, "%s: returned %d, expected 1\n", what, got);
    }
}

static tm_store store(void* p) {
    tm_store s;
    std::memset(&s, 0, sizeof s);
    s.n_games = 8; s.app = 1;
    s.env_game = (uint32_t*)p; s.env_line_stats = (int32_t*)p;
    return s;
}

int main() {
    alignas(16) static char buf[64];
    uint32_t* up = (uint32_t*)buf;
    int32_t* ip = (int32_t*)buf;
    tm_store s = store(buf);
    for (int off = 1; off <= 3; ++off) {
        uint32_t* uo = (uint32_t*)(buf + off);
        int32_t* io = (int32_t*)(buf + off);
        expect(tm_env_check(uo, ip, 8, 1, ip, ip, nullptr), "tm_env_check games alignment");
        expect(tm_env_check(up, io, 8, 1, ip, ip, nullptr), "tm_env_check line_stats alignment");
        expect(tm_env_check(up, ip, 8, 1, io, ip, nullptr), "tm_env_check fault alignment");
        expect(tm_env_check(up, nullptr, 8, 1, ip, io, nullptr), "tm_env_check n_bad alignment");
        expect(tm_env_save(&s, uo, ip, nullptr), "tm_env_save games alignment");
        expect(tm_env_save(&s, up, io, nullptr), "tm_env_save line_stats alignment");
        expect(tm_env_load(&s, uo, ip, ip, ip, nullptr), "tm_env_load games alignment");
        expect(tm_env_load(&s, up, io, ip, ip, nullptr), "tm_env_load line_stats alignment");
        expect(tm_env_load(&s, up, ip, io, ip, nullptr), "tm_env_load fault alignment");
        expect(tm_env_load(&s, up, ip, ip, io, nullptr), "tm_env_load n_bad alignment");
        expect(tm_episode_resume(8, 0, io, ip, ip, nullptr), "tm_episode_resume move_idx alignment");
        expect(tm_episode_resume(8, 0, ip, io, ip, nullptr), "tm_episode_resume slot_state alignment");
        expect(tm_episode_resume(8, 0, ip, ip, io, nullptr), "tm_episode_resume counters alignment");
    }
    expect(tm_env_check(nullptr, ip, 8, 1, ip, ip, nullptr), "tm_env_check games");
    expect(tm_env_check(up, ip, 8, 1, nullptr, ip, nullptr), "tm_env_check fault");
    expect(tm_env_check(up, ip, 8, 1, ip, nullptr, nullptr), "tm_env_check n_bad");
    expect(tm_env_check(up, ip, 0, 1, ip, ip, nullptr), "tm_env_check n == 0");
    expect(tm_env_check(up, ip, INT32_MIN, 1, ip, ip, nullptr), "tm_env_check n < 0");
    expect(tm_env_check(up, ip, 8, 0, ip, ip, nullptr), "tm_env_check app == 0");
    expect(tm_env_check(up, nullptr, 8, -1, ip, ip, nullptr), "tm_env_check app < 0");
    expect(tm_env_save(nullptr, up, ip, nullptr), "tm_env_save store");
    expect(tm_env_save(&s, nullptr, ip, nullptr), "tm_env_save games");
    expect(tm_env_save(&s, up, nullptr, nullptr), "tm_env_save line_stats");
    expect(tm_env_load(nullptr, up, ip, ip, ip, nullptr), "tm_env_load store");
    expect(tm_env_load(&s, nullptr, ip, ip, ip, nullptr), "tm_env_load games");
    expect(tm_env_load(&s, up, nullptr, ip, ip, nullptr), "tm_env_load line_stats");
    expect(tm_env_load(&s, up, ip, nullptr, ip, nullptr), "tm_env_load fault");
    expect(tm_env_load(&s, up, ip, ip, nullptr, nullptr), "tm_env_load n_bad");
    {
        tm_store a = store(buf), b = store(buf), c = store(buf), d = store(buf), e = store(buf);
        a.n_games = 0; b.n_games = -4; c.env_game = nullptr; d.env_line_stats = nullptr; e.app = 0;
        expect(tm_env_save(&a, up, ip, nullptr), "tm_env_save n_games == 0");
        expect(tm_env_save(&b, up, ip, nullptr), "tm_env_save n_games < 0");
        expect(tm_env_save(&c, up, ip, nullptr), "tm_env_save env_game");
        expect(tm_env_save(&d, up, ip, nullptr), "tm_env_save env_line_stats");
        expect(tm_env_load(&a, up, ip, ip, ip, nullptr), "tm_env_load n_games == 0");
        expect(tm_env_load(&b, up, ip, ip, ip, nullptr), "tm_env_load n_games < 0");
        expect(tm_env_load(&c, up, ip, ip, ip, nullptr), "tm_env_load env_game");
        expect(tm_env_load(&d, up, ip, ip, ip, nullptr), "tm_env_load env_line_stats");
        expect(tm_env_load(&e, up, ip, ip, ip, nullptr), "tm_env_load app == 0");
    }
    expect(tm_episode_resume(0, 0, ip, ip, ip, nullptr), "tm_episode_resume n_games == 0");
    expect(tm_episode_resume(-1, 0, ip, ip, ip, nullptr), "tm_episode_resume n_games < 0");
    expect(tm_episode_resume(8, -1, ip, ip, ip, nullptr), "tm_episode_resume first_id < 0");
    expect(tm_episode_resume(8, 0, nullptr, ip, ip, nullptr), "tm_episode_resume move_idx");
    expect(tm_episode_resume(8, 0, ip, nullptr, ip, nullptr), "tm_episode_resume slot_state");
    expect(tm_episode_resume(8, 0, ip, ip, nullptr, nullptr), "tm_episode_resume counters");
    std::printf("games_snapshot refusals: %d checked, %d failed\n", n_checked, n_failed);
    return n_failed ? 1 : 0;
}
