"""k_vn_conv_fc1's stations in time (a -DTM_FUSED_TIMELINE build of valuenet.hip, linked with the other objects into a library of its
own): s_memrealtime (100 MHz) of every workgroup at the launch's entry, when its wave 0 reaches the wait of its first item (out of
phase 1, the item's weights, biases and request slots requested), when it sees the tile ready, behind the barrier (the whole
workgroup out of phase 1), fc1's stations as scripts/fc1_timeline.py, and the end of every convolution wave's state.  The list: a
4 096-game ValueSim store a move into play, one launch of the tree kernel, the first B requests of it (the request cap).
    TETRIS_MCTS_LIB=<that library> python scripts/fused_timeline.py [B=1867] [out.json]"""
import json, os, sys
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tetris_mcts_amd import agents, store as st  # noqa: E402
from tetris_mcts_amd.model import Model_VV  # noqa: E402
from tetris_mcts_amd.pyTetris import Tetris  # noqa: E402
B = int(sys.argv[1]) if len(sys.argv) > 1 else 1867
G, env_args = 4096, ((20, 10), 1, 0, 0)
m = Model_VV(backend="hip", seed=0)
game = Tetris(*env_args, seed=100, n_games=G)
agent = agents.ValueSim(sims=8, env=Tetris, env_args=env_args, n_games=G, max_nodes=4096, model=m, online=False)
agent.update_root(game)
game.play(agent.play())
agent.update_root(game)
s = agent.store
s.move_begin(4)
s.sim_step(st.SIM_BACKUP | st.SIM_FRONT)
posted = int(s.t["eval_cnt"][:, s.s.eval_parity].sum().item())
assert posted >= B, posted
s.s.eval_cap, s.s.eval_rot = B, 0
u = lambda a: a.astype(np.uint32).astype(np.int64)  # noqa: E731
pc = lambda x: [round(float(x.mean()), 2), round(float(np.percentile(x, 50)), 2), round(float(x.min()), 2), round(float(x.max()), 2)]  # noqa: E731
rows = []
for it in range(6):
    m._scratch.zero_()
    m.inference_requests(s)
    torch.cuda.synchronize()
    sc = m._scratch[:B].view(torch.int32).cpu().numpy()
    pad = u(sc[:, 2048:2064])
    conv_end = pad[:, 13]
    assert (conv_end != 0).all()
    tiles = (B + 31) // 32
    it_rows = [t * 32 + y for t in range(tiles) for y in range(4) if t * 32 + y < B]
    w = pad[it_rows]                                  # one row per item = per workgroup (B <= 2 048: an item a workgroup at most)
    tile_last = np.array([conv_end[r // 32 * 32:min(r // 32 * 32 + 32, B)].max() for r in it_rows])
    ref = w[:, 9].min()
    us = lambda x: (x - ref) / 100.0  # noqa: E731
    all_conv = conv_end.max()
    row = {"requests": B, "workgroups_with_an_item": len(it_rows),
           "last_convolution_wave_ended": round(float(us(all_conv)), 2),
           "wave0_at_its_wait": pc(us(w[:, 10])), "tile_ready_seen": pc(us(w[:, 11])), "workgroup_out_of_phase_1": pc(us(w[:, 12])),
           "first_chunk_requested": pc(us(w[:, 2])), "first_chunk_staged": pc(us(w[:, 3])), "k_loop_done": pc(us(w[:, 4])),
           "arrived": pc(us(w[:, 6])),
           "ready_seen_after_the_tiles_last_row_us": pc((w[:, 11] - tile_last) / 100.0),
           "staged_after_ready_seen_us": pc((w[:, 3] - w[:, 11]) / 100.0),
           "staged_after_the_tiles_last_row_us": pc((w[:, 3] - tile_last) / 100.0),
           "staged_after_the_last_convolution_wave_us": pc((w[:, 3] - all_conv) / 100.0),
           "waited_us": pc((w[:, 11] - w[:, 10]) / 100.0),
           "k_loop_us": pc((w[:, 4] - w[:, 3]) / 100.0)}
    if it >= 2:
        rows.append(row)
        print(json.dumps(row), flush=True)
if len(sys.argv) > 2:
    json.dump({"what": __doc__, "columns": "mean, median, min, max over the workgroups that hold an item; microseconds after the launch's first entry unless named _us",
               "rows": rows}, open(sys.argv[2], "w"), indent=1)
