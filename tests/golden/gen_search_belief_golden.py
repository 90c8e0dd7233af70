"""Generates tests/golden/search_belief_lastmove.json: the games SearchPlayer(condition=True) plays (tests/search_util.py's
_conditioned_games), recorded on the GPU at the commit before hb_belief_splice / hb_belief_select became the alive = NULL /
depth = 1 cases of hb_belief_splice_alive / hb_belief_select_depth. Philox draws and integer sums only, so two runs write the
same bytes. An optional argument names another output file."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "hanabi-agents_amd"), os.path.dirname(HERE)):
    sys.path.insert(0, p)
from search_util import _conditioned_games  # noqa: E402


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "search_belief_lastmove.json")
    with open(path, "w") as f:
        json.dump(_conditioned_games(), f, separators=(",", ":"))
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
