#!/usr/bin/env python3
"""Analyse a position: play a few moves with GoEnv, search the position with a (random-weight) network and print what the
search thinks -- per candidate move its visits, value and prior, and the line it expects.

    python examples/analyse_position.py            # needs an MI355X; a few seconds
    python examples/analyse_position.py --symmetry mean8 --playouts 64
    python examples/analyse_position.py --ownership    # who owns what, and black's lead, averaged over the searched positions
    python examples/analyse_position.py --pass-alive   # a column `pa`: what is settled by proof (pass-alive stones and territory)
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from transgo_amd import analysis, model                           # noqa: E402
from transgo_amd.engine import SelfPlayEngine                     # noqa: E402
from transgo_amd.environment import GoEnv                         # noqa: E402


def main(moves=("E5", "C3", "G7", "C7"), sims=200, filters=32, blocks=2, board_size=9, playouts=0, symmetry="none", ownership=False,
         pass_alive=False):
    env = GoEnv(board_size=board_size)
    state, _ = env.reset()
    names = {analysis.vertex(a, board_size): a for a in range(board_size ** 2 + 1)}
    for m in moves:
        state, done = env.step(state, names[m])
        assert not done
    env.show(state)
    eng = SelfPlayEngine(1, board_size=board_size, num_simulation=sims, net_blocks=blocks, net_filters=filters)
    model.load_into(eng.ctx, model.random_weights(board_size, 10, filters, blocks, seed=3), board_size, 10, filters, blocks)
    eng.reset([0])                                                # seeds the stream the search's tie breaks draw from
    # --symmetry position | mean8: evaluate every leaf in one orientation chosen from the position, or as the mean over all eight
    # --ownership: the search also averages the ownership head over the positions it evaluates; the record's board is printed too
    rec = analysis.analyse(eng, np.frombuffer(state, np.uint8).reshape(1, -1), symmetry=symmetry, ownership=ownership,
                           pass_alive=pass_alive)[0]
    # --playouts N: the network-free Monte-Carlo ownership / score estimate next to the search (N random games in one launch)
    own = analysis.playout_ownership(env, np.frombuffer(state, np.uint8).reshape(1, -1), playouts=playouts)[0] if playouts else None
    print(analysis.format_analysis(rec, board_size, top=8, ownership=own))
    eng.close()
    return rec


if __name__ == "__main__":
    sym = sys.argv[sys.argv.index("--symmetry") + 1] if "--symmetry" in sys.argv else "none"
    if sym not in ("none", "position", "mean8"):
        sys.exit("--symmetry takes none, position or mean8")
    main(playouts=int(sys.argv[sys.argv.index("--playouts") + 1]) if "--playouts" in sys.argv else 0, symmetry=sym,
         ownership="--ownership" in sys.argv, pass_alive="--pass-alive" in sys.argv)
