"""The scale-up preview's reference (tests/scaleup_ref.py) on the shared 32-node trace, on the CPU: an
option is the placement reference on the concatenated arrays, so an option without nodes is the plain
placement preview, and asking again with exactly the nodes an option used changes no placement."""
import numpy as np
import pytest

import place_ref as pr
import scaleup_ref as sr
from harness import MODES

TICKS = (0, 137, 800)


def case_state(r, t):
    return sr.state_before(r["fast"][t], r["shapes"], r["shape_of"])


@pytest.mark.parametrize("case", ["feeds", "literal", "feeds_irregular"])
def test_options_on_the_shared_trace(case):
    r = pr.parity_case(case)
    enc = r["enc"]
    n = len(enc["alloc"])
    cfg = pr.engine_cfg(MODES[r["mode"]], enc)
    opts = sr.trace_options(enc)
    on_new, on_old = 0, 0
    for t in TICKS:
        state = case_state(r, t)
        res = sr.scale_up(enc["alloc"], state, cfg, r["shapes"], r["shape_of"], opts)
        # no appended node: the plain preview (which also pins the state rebuilt from the binds)
        for f in sr.ROWS:
            np.testing.assert_array_equal(res[3][f], r["fast"][t][f], err_msg=f"{case} tick {t}: {f}")
        assert res[3]["summary"]["on_new"] == 0 and res[3]["summary"]["nodes_used"] == 0
        for g, (o, w) in enumerate(zip(opts, res)):
            s = w["summary"]
            assert s["ok"] + s["over_capacity"] + s["not_found"] == pr.N_PODS
            assert s["nodes_used"] <= min(o["max_nodes"], s["on_new"])
            on_new += s["on_new"]
            on_old += s["ok"] - s["on_new"]
            # exactly the nodes that were used: the same placements (candidates count the unused ones)
            hi = sr.highest_used(w, n)
            again = sr.scale_up_one(enc["alloc"], state, cfg, r["shapes"], r["shape_of"], dict(o, max_nodes=hi + 1))
            for f in ("node", "status", "score"):
                np.testing.assert_array_equal(again[f], w[f], err_msg=f"{case} tick {t} option {g}: {f}")
            assert again["summary"] == s
            # appended nodes fill in index order: the used ones are a prefix
            used = sorted(set(w["node"][w["node"] >= n].tolist()))
            assert used == list(range(n, n + len(used)))
    assert on_new >= 20 and on_old >= 20, (on_new, on_old)
