"""What the backups' shifts look like in every regime of tests/dist_regimes.py and at the suite's own setting (50 atoms over
[0, 5000)): the oracle alone, its per-agent census (oracle.Agent.dist_census) summed over the games.  CPU only.

    python scripts/dist_regimes_census.py [out.json]        (default: profiles/dist_regimes_census.json)
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import dist_regimes as R  # noqa: E402
from oracle import binding  # noqa: E402


def main(out):
    binding.lib()
    rows = []
    for r in R.REGIMES + (R.SUITE_SETTING,):
        row = dict(r._asdict(), games=R.GAMES, seed0=R.SEED0, low=R.LOW, scoring=R.SCORING, randomizer=R.RANDOMIZER)
        row["census"] = R.census(binding, r)
        rows.append(row)
        print(r.name, row["census"])
    with open(out, "w") as f:
        json.dump(rows, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "dist_regimes_census.json"))
