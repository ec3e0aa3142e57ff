"""The inputs of tests/test_preview_wide_gpu.py, pinned on the references alone
(tests/preview_wide_cases.py): the wide clusters put winners into block lists that one lane of
place_merge_kernel folds on its second and third trip, ties among them, short complete lists in the
high blocks, calls of two rounds, cordons over the bitmap's word 512 and its last word; the long
history keeps a running pod in more than 256 gather blocks, on both sides of drain_scan_kernel's chunk
edge.  A case that misses its condition is changed in preview_wide_cases.py; the conditions here stay.

One condition is stated otherwise than planned: at 65 scan blocks the only two blocks one lane folds
are 0 and 64, so the pair there is (0, 64); a pair that leaves block 0 out is asserted at 129 blocks.
"""
import os
import re

import numpy as np
import pytest

import consolidate_ref as cr
import place_ref as pr
import preview_wide_cases as wc
import removable_ref as rr

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "kubernetes-simulator_amd", "csrc")
FEEDS_CASES = ("b64", "b65", "b65_idle", "b129")
L, BLK, WAVE = wc.L, wc.BLK, wc.WAVE


def _high_idle(name):
    """whether idle planted nodes lie past block 63: at 65 blocks block 64 is one node, which either runs
    pods ("host") or idles behind the taint ("idle")"""
    return wc.wide_case(name)["nblk"] > 2 * WAVE or (wc.wide_case(name)["nblk"] > WAVE and wc.WIDE[name][2] == "idle")


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def test_the_restated_constants_are_the_sources():
    dev, qry, place, drain = _src("ks_device.h"), _src("ks_query.h"), _src("ks_place.hip"), _src("ks_drain.hip")
    assert int(re.search(r"#define\s+KS_PLACE_L\s+(\d+)", qry).group(1)) == L == 32
    assert int(re.search(r"constexpr int kPBlk = (\d+);", place).group(1)) == BLK
    assert int(re.search(r"constexpr int kDrainBlk = (\d+);", qry).group(1)) == BLK
    assert "b += kWave" in place and re.search(r"constexpr int kWave = (\d+);", dev).group(1) == str(WAVE)
    assert "base += kDrainBlk" in drain, "the gather's scan no longer walks chunks of kDrainBlk counts"
    assert [wc.WIDE[c][0] for c in FEEDS_CASES] == [16_384, 16_385, 16_385, 32_770]
    assert [wc.wide_case(c)["nblk"] for c in FEEDS_CASES] == [64, 65, 65, 129]
    assert all(wc.WIDE[c][1] == pr.FEEDS for c in FEEDS_CASES) and wc.WIDE["b65_literal"][:2] == (16_385, pr.LITERAL)


def _winner_blocks(name):
    """per shape the winners (the first L nodes by score, then index) and their totals on the last tick"""
    c = wc.wide_case(name)
    V = wc.score_vectors(c, wc.T_WIDE)
    return [(wc.winners(v), v) for v in V]


def _same_lane_tie(w, v):
    """a pair of winners with the same total in two different blocks that one lane folds"""
    for i in range(len(w)):
        for j in range(i + 1, len(w)):
            bi, bj = int(w[i]) // BLK, int(w[j]) // BLK
            if v[w[i]] == v[w[j]] and bi != bj and (bj - bi) % WAVE == 0:
                return int(w[i]), int(w[j])
    return None


@pytest.mark.parametrize("name", list(wc.WIDE))
def test_the_run_leaves_pods_on_high_nodes(name):
    c = wc.wide_case(name)
    assert len(c["ob"]["pod"]) == wc.N_TRACE - wc.N_LATER and len(c["nxt"]["pod"]) == wc.N_LATER >= 20
    assert c["ob"]["tick"].max() < wc.T_WIDE - 100 and c["nxt"]["tick"].min() > wc.T_WIDE
    if c["mode"] == pr.FEEDS:
        assert (c["ob"]["status"] == 0).all()
    else:
        assert (c["ob"]["status"] == 1).sum() >= 50, "the literal run refuses few pods"
    for t in (wc.T_PAST, wc.T_WIDE):
        run = c["state"][t][:, 3]
        assert run.sum() >= (100 if c["mode"] == pr.FEEDS else 20)
        if c["mode"] == pr.FEEDS:
            want = {x // BLK for x in c["plant"]["host"]}
            assert {0, 63} <= want and len(want) == (2 if name in ("b64", "b65_idle") else 3 if name == "b65" else 5)
            assert want <= set((np.nonzero(run)[0] // BLK).tolist()), "a planted block runs no pod"
    differ = (c["state"][wc.T_PAST] != c["state"][wc.T_WIDE]).any(axis=1).sum()   # the past tick is another state
    assert differ >= (10 if c["mode"] == pr.FEEDS else 5)


@pytest.mark.parametrize("name", list(wc.WIDE))
def test_winners_come_from_lists_one_lane_folds_in_several_trips(name):
    c = wc.wide_case(name)
    nblk, last = c["nblk"], c["nblk"] - 1
    per = _winner_blocks(name)
    pairs, triples, in_last, ties = [], [], [], []
    for j, (w, v) in enumerate(per):
        blocks = set((w // BLK).tolist())
        pairs += [(j, b, b + WAVE) for b in sorted(blocks) if b + WAVE in blocks]
        triples += [(j, b) for b in sorted(blocks) if b + WAVE in blocks and b + 2 * WAVE in blocks]
        in_last += [j] if last in blocks else []
        tie = _same_lane_tie(w, v)
        ties += [(j,) + tie] if tie else []
    print(name, "pairs", pairs, "triples", triples, "last block in", in_last, "ties", ties)
    assert in_last, "no shape's winners hold a node of the last block"
    if nblk > WAVE:
        assert (c["n"] - last * BLK) < BLK, "the last block is not ragged"
        assert pairs, "no shape's winners hold nodes of two blocks one lane folds"
    if _high_idle(name):
        assert ties, "no tie between two blocks of one lane among the winners"
        # the lower index wins it: the reference's order
        j, lo, hi = ties[0]
        w = per[j][0].tolist()
        assert lo < hi and w.index(lo) < w.index(hi)
    if nblk > 2 * WAVE:
        assert any(b >= 1 for _, b, _ in pairs), "every pair holds block 0"
        assert triples, "no shape's winners hold b, b + 64 and b + 128"
    if nblk <= WAVE:
        assert not pairs and len(set((per[wc.TIE][0] // BLK).tolist())) >= 4


@pytest.mark.parametrize("name", FEEDS_CASES)
def test_short_lists_full_counts_and_two_rounds(name):
    c = wc.wide_case(name)
    nblk = c["nblk"]
    V = wc.score_vectors(c, wc.T_WIDE)
    short = np.nonzero(V[wc.SHORT])[0]
    lo = WAVE if nblk > WAVE else WAVE // 2
    print(name, "short list", short.tolist())
    assert 1 <= len(short) < L and (short // BLK >= lo).all(), "the short list is not short, or not high"
    every = [j for j in range(len(V)) if len(set((np.nonzero(V[j])[0] // BLK).tolist())) == nblk]
    assert every, "no shape counts candidates in every block"
    assert (V[7] == 0).all() and 0 < (V[wc.PLAIN] > 0).sum() < (V[wc.SMALL] > 0).sum() <= c["n"]
    # more than L candidates behind the wide gate, and its copies land on more nodes than a list holds:
    # winners are list entries, so the (L + 1)-th distinct node needs a second round's lists
    assert (V[wc.GATED] > 0).sum() > L
    r = wc.copies_ref(name)
    assert (r["status"] == pr.OK).all() and len(set(r["node"].tolist())) > L
    if _high_idle(name):
        assert (r["node"] // BLK >= WAVE).any(), "no copy lands past block 63"


@pytest.mark.parametrize("name", list(wc.WIDE))
def test_the_placements_use_the_high_blocks(name):
    c = wc.wide_case(name)
    nblk = c["nblk"]
    for t in (wc.T_PAST, wc.T_WIDE):
        r = wc.place_ref(name, t)
        blocks = set((r["node"][r["node"] >= 0] // BLK).tolist())
        print(name, t, "blocks", sorted(blocks), "info", r["info"], "reused", len(r["reused"]))
        # (with the filters ignored the pods pile on the full one-pod nodes: fewer nodes, refused binds)
        assert len(blocks) >= (3 if c["mode"] == pr.FEEDS else 2)
        assert len(set(r["node"].tolist())) >= (12 if c["mode"] == pr.FEEDS else 4)
        if c["mode"] == pr.FEEDS:
            assert nblk - 1 in blocks, "no placement in the last block"
            assert r["info"][3] == wc.N_PODS // 8 and (r["candidates"][r["status"] == pr.NOT_FOUND] == 0).all()
            assert len(set(r["candidates"].tolist())) >= 6
        else:
            assert (r["candidates"] == c["n"]).all() and (r["status"] == pr.OVER).sum() >= 1
    assert any(wc.place_ref(name, wc.T_PAST)[f].tolist() != wc.place_ref(name, wc.T_WIDE)[f].tolist()
               for f in ("node", "score")), "the past tick asks nothing new"


@pytest.mark.parametrize("name", list(wc.WIDE))
def test_the_drained_set_mixes_hosts_idle_winners_and_the_tie(name):
    c = wc.wide_case(name)
    nblk, last = c["nblk"], c["nblk"] - 1
    nodes, run = wc.drain_nodes(name), c["state"][wc.T_WIDE][:, 3]
    d = wc.drain_ref(name)
    print(name, "drained", nodes, "evicted", len(d["pod"]), "to blocks", sorted(set((d["node"] // BLK).tolist())))
    if c["mode"] == pr.FEEDS:
        busy = {x // BLK for x in nodes if run[x] > 0}
        assert {x // BLK for x in c["plant"]["host"]} <= busy
        words = {x // 32 for x in nodes}
        if nblk > WAVE:
            assert 512 in words, "no drained node in the cordon's word 512"
        if nblk > 2 * WAVE:
            assert (c["n"] - 1) // 32 in words, "no drained node in the cordon's last word"
        # idle nodes that head the evicted pods' lists: every evicted shape's un-cordoned winners hold one
        idle = [x for x in nodes if x in c["plant"]["reserve"]]
        assert len(idle) >= 2 and (run[idle] == 0).all()
        rest = [x for x in wc.idle_reserve(c, wc.T_WIDE) if x not in nodes]
        assert rest, "no idle reserve node is left to receive a pod"
        assert idle[0] == wc.idle_reserve(c, wc.T_WIDE)[0], "the tie's winner (the lowest idle reserve node) stays"
        if nblk > 2 * WAVE:    # (at 65 blocks the only second-trip block is one node: a host, or behind the taint)
            assert any(x // BLK >= WAVE for x in idle), "no drained idle winner in a second-trip block"
        assert set(d["node"].tolist()) & set(rest), "no evicted pod moves to an idle node that was left"
        assert c["plant"]["idle"][0] in nodes and len(d["pod"]) >= 15 and d["info"][1] == len(d["pod"])
        assert d["info"][5] >= 3
    else:
        assert len(d["pod"]) >= 4 and d["info"][1] >= 1
    assert (np.diff(d["pod"]) > 0).all() and not set(d["node"].tolist()) & set(nodes)


@pytest.mark.parametrize("name", list(wc.WIDE))
def test_the_candidates_are_permuted_and_one_is_an_entry_of_a_high_list(name):
    c = wc.wide_case(name)
    cand = wc.candidates(name)
    assert len(cand) == len(set(cand)) and 19 <= len(cand) <= 24 and list(cand) != sorted(cand)
    assert set(wc.drain_nodes(name)) <= set(cand) or len(cand) == 24
    rm, co = wc.removable_ref(name), wc.consolidate_ref(name)
    print(name, "evicted", rm["evicted"].tolist(), "outcome", co["outcome"].tolist(), co["info"])
    assert rm["evicted"].max() < L, "a candidate takes the single path: the lists are not used"
    assert (rm["evicted"] == 0).sum() >= 3 and (rm["evicted"] > 0).sum() >= (6 if c["mode"] == pr.FEEDS else 3)
    ranks = rr.own_node_ranks(c["enc"], c["cfg"], c["state"][wc.T_WIDE], rm, L)
    own = (ranks >= 0) & (ranks < L)
    high = own & (rm["rows"]["from_node"] // BLK >= (WAVE if c["nblk"] > WAVE else WAVE // 2))
    print(name, "pods whose own node is in their list", int(own.sum()), "of them on a high block", int(high.sum()))
    assert own.any()
    if c["mode"] == pr.FEEDS:
        if wc.WIDE[name][2] == "host":
            assert high.any(), "no candidate is an entry of a high block's list"
        assert co["info"][1] >= 5 and co["info"][3] >= 3 and co["info"][5] >= 20
        assert (co["outcome"] != cr.REMOVED).any() and rm["removable"].all()


@pytest.mark.parametrize("name", list(wc.WIDE))
def test_the_scale_up_options(name):
    c = wc.wide_case(name)
    n, opts, ref = c["n"], wc.scale_options(c), wc.scale_ref(name)
    assert len(opts) == 4 and len(wc.SCALE_OF) <= 1024 and len(wc.SCALE_SHAPES) <= 8
    for o in opts[:2]:
        assert n // BLK != (n + o["max_nodes"] - 1) // BLK, "the appended nodes stay inside one scan block"
    print(name, [r["summary"] for r in ref])
    plain = wc.scale_place_ref(name)
    for f in pr.FIELDS:                                    # the option that appends nothing is place_at
        np.testing.assert_array_equal(ref[2][f], plain[f])
    if c["mode"] == pr.FEEDS:
        k = len(wc.SCALE_OF)
        assert ref[0]["summary"]["on_new"] >= k - 12 and ref[0]["summary"]["on_new"] > ref[1]["summary"]["on_new"]
        on_real = ref[1]["node"][(ref[1]["node"] >= 0) & (ref[1]["node"] < n)]
        assert len(on_real) >= 8, "the mid-sized template loses nowhere"
        if _high_idle(name):
            assert (on_real // BLK >= WAVE).any(), "the mid-sized template loses to no node past block 63"
        assert ref[3]["summary"]["nodes_used"] == 7 and ref[3]["summary"]["on_new"] == 14


# ---- depth ---------------------------------------------------------------------------------------
def test_the_long_history_keeps_a_pod_running_in_more_than_256_blocks():
    c = wc.deep_case()
    ob, s = c["ob"], c["stragglers"]
    assert len(ob["pod"]) == wc.DEEP_PODS >= 66_048 and (ob["status"] == 0).all()
    np.testing.assert_array_equal(ob["tick"], 1 + np.arange(wc.DEEP_PODS))
    assert len(set((s // BLK).tolist())) == wc.DEEP_BLOCKS >= 258
    lanes = {int(q) % BLK for q in s}
    assert set(wc.LANES) <= lanes
    for b in (255, 256):
        assert {b * BLK + o for o in wc.LANES} <= set(s.tolist())
    assert ((s // BLK) == wc.TRIPLE_BLOCK).sum() >= 3 and wc.TRIPLE_BLOCK >= 256
    late, early = wc.deep_running_blocks(wc.DEEP_LATE), wc.deep_running_blocks(wc.DEEP_EARLY)
    print("blocks with a running pod: late", len(late), "early", len(early))
    assert len(late) == wc.DEEP_BLOCKS > 256 and late.tolist() == list(range(wc.DEEP_BLOCKS))
    assert 100 < len(early) < 256
    # every pod that is no straggler has ended long before either tick's last 100 binds
    ref = c["ref"]
    short = ~np.isin(ref.pod, s)
    assert (ref.e[short] - ref.b[short]).max() <= 3 and (ref.e[~short] > wc.DEEP_T + 1000).all()


@pytest.mark.parametrize("t", [wc.DEEP_LATE, wc.DEEP_EARLY])
def test_the_drained_nodes_evict_on_both_sides_of_the_chunk_edge(t):
    r = wc.deep_refs(t)
    d, nodes = r["drain"], r["nodes"]
    blocks = sorted(set((d["pod"] // BLK).tolist()))
    print("tick", t, "nodes", nodes, "evicted", len(d["pod"]), "blocks", len(blocks), "first", blocks[:3], "last", blocks[-3:])
    assert len(nodes) >= 4 and len(set(nodes)) == len(nodes)
    assert (np.diff(d["pod"]) > 0).all(), "the expected eviction list is not in ascending pod order"
    assert len(d["pod"]) >= 12 and d["info"][1] == len(d["pod"])
    if t == wc.DEEP_LATE:
        assert min(blocks) < 255 and 255 in blocks and 256 in blocks and wc.TRIPLE_BLOCK in blocks
        assert (d["pod"] // BLK == wc.TRIPLE_BLOCK).sum() >= 3
        assert {255 * BLK + o for o in wc.LANES} & set(d["pod"].tolist()) and {256 * BLK + o for o in wc.LANES} & set(d["pod"].tolist())
    else:
        assert max(blocks) < 256
    rm = r["removable"]
    assert rm["evicted"].sum() == len(d["pod"]) and (rm["evicted"] >= 1).sum() >= 3
    a, b = r["consolidate"]
    assert a["info"][1] >= 1 and b["info"][1] >= 1
    assert a["outcome"].tolist() != b["outcome"][::-1].tolist() or a["rows"]["node"].tolist() != b["rows"]["node"].tolist(), \
        "the second order asks nothing new"
