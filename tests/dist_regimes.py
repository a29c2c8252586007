"""The regimes in which the distributional agent is held to the oracle away from its default 50 atoms over [0, 5000).

At the default one bin is 100 points wide and a backup's reward difference is a few dozen points, so the shift of the leaf's
distribution (agents/core_distributional.py shift_distribution; tree.hip wave_dist_back writes it as a gather) almost never
moves mass by a whole bin.  Each row below narrows the bins until the shifts the default never produces are the common case;
tests/test_oracle_dist.py proves that on the CPU with the oracle's census (oracle.Agent.dist_census), and
tests/test_gpu_dist_agent.py holds the device to the oracle bit for bit in the same runs.  Plain data plus the helper that
builds the oracle side; nothing here needs a GPU."""
from collections import namedtuple

Regime = namedtuple("Regime", "name atoms vmin vmax app moves sims max_nodes")

SCORING, RANDOMIZER, LOW, GAMES, SEED0 = 0, 0, 5, 6, 4242

REGIMES = (
    # bins one point wide and integer rewards: every non-zero shift is a whole number of bins, many beyond the top
    Regime("whole", 50, 0.0, 50.0, 1, 10, 100, 5000),
    # delta = 7/3: b + bin_shift rounds up across an integer for some source bins (x = 35 -> 14.999999999999998)
    Regime("round", 30, 0.0, 70.0, 1, 10, 100, 5000),
    # the same arithmetic through the backup's sequential branch (app != 1)
    Regime("round_app3", 30, 0.0, 70.0, 3, 12, 100, 5000),
    # delta = 0.14: nearly every shift passes the top; rounded sources; the sequential branch
    Regime("tiny_app2", 50, 0.0, 7.0, 2, 10, 100, 5000),
    # the whole wave: one lane per atom at 64 atoms, bins half a point wide
    Regime("full_wave", 64, 0.0, 32.0, 1, 10, 100, 5000),
    Regime("one", 1, 0.0, 10.0, 1, 10, 100, 5000),
    Regime("two", 2, 0.0, 100.0, 1, 10, 100, 5000),
    # atom counts that are no multiple of anything, fractional shifts of one bin and more
    Regime("seven", 7, 0.0, 300.0, 1, 10, 100, 5000),
    Regime("odd", 63, 0.0, 1000.0, 1, 10, 100, 5000),
    # vmin != 0: delta = 10
    Regime("offset", 50, -100.0, 400.0, 1, 10, 100, 5000),
)
BY_NAME = {r.name: r for r in REGIMES}
# what every other test of the distributional tree kernels runs: the agent's defaults
SUITE_SETTING = Regime("suite", 50, 0.0, 5000.0, 1, 10, 100, 5000)


def env_args(regime):
    return ((20, 10), regime.app, SCORING, RANDOMIZER)


def seeds(n_games=GAMES, seed0=SEED0):
    return [seed0 + g for g in range(n_games)]


def oracle_side(oracle, regime, max_nodes=None, n_games=GAMES, seed0=SEED0, **agent_kwargs):
    """(games, agents) of the oracle for a regime: one kind-6 agent per game, rooted at its game"""
    max_nodes = regime.max_nodes if max_nodes is None else max_nodes
    og = [oracle.Game(app=regime.app, scoring=SCORING, randomizer=RANDOMIZER, seed=s) for s in seeds(n_games, seed0)]
    oa = [oracle.Agent(6, max_nodes=max_nodes, app=regime.app, scoring=SCORING, randomizer=RANDOMIZER, low=LOW,
                       dist_bins=regime.atoms, dist_vmin=regime.vmin, dist_vmax=regime.vmax, **agent_kwargs) for _ in range(n_games)]
    for g, a in zip(og, oa):
        a.update_root(g)
    return og, oa


def oracle_step(og, oa, g, action):
    """game g of the oracle side takes `action`; a finished game starts again"""
    og[g].play(action)
    oa[g].update_root(og[g])
    if og[g].end:
        og[g].reset()
        oa[g].update_root(og[g])


def census(oracle, regime, moves=None, sims=None, max_nodes=None):
    """the oracle alone over a regime: the agents' censuses summed (the longest trace: their maximum)"""
    moves = regime.moves if moves is None else moves
    sims = regime.sims if sims is None else sims
    og, oa = oracle_side(oracle, regime, max_nodes)
    for _ in range(moves):
        for g in range(len(oa)):
            a = oa[g].play(sims)
            assert oa[g].error == 0, (regime.name, g, oa[g].error)
            oracle_step(og, oa, g, a)
    total = dict.fromkeys(oracle.Agent.DIST_CENSUS, 0)
    for a in oa:
        for k, v in a.dist_census().items():
            total[k] = max(total[k], v) if k == "longest_trace" else total[k] + v
    total["n_gc"] = sum(a.n_gc for a in oa)
    return total
