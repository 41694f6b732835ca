"""What the case tables of tests/norm_forms.py cover, asserted through the host-only plan query (no GPU): every GroupNorm launch
form, 1 / 2 / 4 groups per block, the B >= 64 fall-through, 1 / 2 / 3 column passes of the chunked form, a block with idle threads,
the seam and pass-boundary cuts the cases are in the table for — so a changed threshold in csrc/norm.hip fails here instead of
quietly leaving tests/test_norm_forms_gpu.py on another kernel."""
import ctypes
import os

import pytest

import norm_forms as nf


@pytest.fixture(scope="module", autouse=True)
def _rule_not_pinned():
    for v in ("ALDM_GN_FUSED_MAX", "ALDM_GN_SPLIT_FUSED"):
        assert v not in os.environ, f"{v} overrides the GroupNorm rule: unset it to test the rule"


@pytest.mark.parametrize("case", nf.GN_CASES, ids=lambda c: c.id)
def test_groupnorm_case_takes_the_form_the_table_says(case):
    pl = case.plan()
    assert (pl["form"], pl["groups_per_block"], pl["passes"], pl["active_threads"]) == (case.form, case.gpb, case.passes, case.active), \
        (case.id, case.why, pl)
    assert pl["group_slices"] * pl["groups_per_block"] == case.G
    assert pl["cols"] * pl["rows"] <= 256 and pl["chunks"] * pl["chunk_px"] >= case.P > (pl["chunks"] - 1) * pl["chunk_px"]
    if case.split_form is None:
        from audioldm2_amd import ops
        with pytest.raises(RuntimeError, match="split image needs"):
            ops.groupnorm_plan(case.B, case.P, case.C1, case.C2, case.G, True)
    else:
        ps = case.plan(True)
        assert ps["form"] == case.split_form, (case.id, ps)
        assert {k: v for k, v in ps.items() if k != "form"} == {k: v for k, v in pl.items() if k != "form"}


def test_groupnorm_table_covers_every_form_and_geometry():
    plans = [(c, c.plan(), c.plan(True) if c.split_form else None) for c in nf.GN_CASES]
    assert {pl["form"] for _, pl, _ in plans} == {"chunked", "fused"}
    assert {ps["form"] for _, _, ps in plans if ps} == {"chunked", "fused", "fused_split"}
    fused = [(c, pl) for c, pl, _ in plans if pl["form"] == "fused"]
    chunked = [(c, pl) for c, pl, _ in plans if pl["form"] == "chunked"]
    assert {pl["groups_per_block"] for _, pl in fused} == {1, 2, 4}
    # the one-launch split at 2 and at 4 groups per block, and the fused statistics + split_rows form at 4
    assert {ps["groups_per_block"] for _, _, ps in plans if ps and ps["form"] == "fused_split"} >= {2, 4}
    assert any(ps and ps["form"] == "fused" and ps["groups_per_block"] == 4 for _, _, ps in plans)
    # B >= 64 with 32 groups: eight groups per block, chunked however small the sample is
    assert any(c.B >= 64 and c.G == 32 and pl["groups_per_block"] == 8 and c.P * c.C <= 1 << 17 and c.P <= 1024 for c, pl in chunked)
    assert {pl["passes"] for _, pl in chunked} == {1, 2, 3}
    assert any(pl["passes"] == 2 for _, pl in fused)                                       # a fused block with > 256 float4 columns
    assert any(pl["active_threads"] < 256 for _, pl in fused) and any(pl["active_threads"] < 256 for _, pl in chunked)
    assert any(c.P < pl["rows"] for c, pl in fused)                                        # fewer pixels than block rows
    assert any(c.P % pl["chunk_px"] and c.P % pl["chunk_px"] < pl["rows"] for c, pl in chunked)   # ragged last chunk under the rows
    assert any(c.P > 1024 for c, _ in chunked) and any(c.P * c.C > 1 << 17 and c.P <= 1024 for c, _ in chunked)
    assert {c.G for c, _ in fused} >= {1, 32, 64} and {c.G for c, _ in chunked} >= {32, 64}
    # a group cut by a pass boundary (chunked: passes of 256 float4 columns from column 0), and by the x1 / x2 seam in both forms
    def cut_by_pass(c, pl):
        cg4 = c.C // c.G // 4
        return any((k * pl["cols"]) % cg4 for k in range(1, pl["passes"]))
    assert sum(cut_by_pass(c, pl) for c, pl in chunked) >= 2
    seam_cut = lambda c: c.C2 and c.C1 % (c.C // c.G) != 0
    assert any(seam_cut(c) for c, _ in fused) and any(seam_cut(c) for c, _ in chunked)
    assert any(seam_cut(c) and ps and ps["form"] == "fused_split" for c, _, ps in plans)
    assert max(c.B * c.P * c.C * 4 for c in nf.GN_CASES) <= 17 << 20                       # the largest input: ~16 MB


def test_spike_positions_reach_every_edge_of_the_plan():
    for c in nf.GN_CASES:
        pl = c.plan()
        pos = nf.spike_positions(c, pl)
        px, ch = {p for p, _ in pos}, {q for _, q in pos}
        assert all(0 <= p < c.P and 0 <= q < c.C for p, q in pos) and len(set(pos)) == len(pos)
        assert {0, c.P - 1} <= px and {0, c.C - 1} <= ch
        if c.C2:
            assert {c.C1 - 1, c.C1} <= ch
        if pl["chunks"] > 1:
            assert {pl["chunk_px"] - 1, (pl["chunks"] - 1) * pl["chunk_px"]} <= px
        if pl["passes"] > 1:
            assert {4 * pl["cols"] - 1, 4 * pl["cols"]} <= ch
        # a pixel of the tail loop wherever a thread's trip count is no multiple of the unroll
        trips = (min(c.P, pl["chunk_px"]) + pl["rows"] - 1) // pl["rows"]
        if trips % nf.GN_UNROLL:
            assert pl["rows"] * nf.GN_UNROLL * (trips // nf.GN_UNROLL) in px
        assert nf.spike_reps(c, pl) * c.B >= len(pos)
    assert any((min(c.P, c.plan()["chunk_px"]) + c.plan()["rows"] - 1) // c.plan()["rows"] % nf.GN_UNROLL for c in nf.GN_CASES)


def test_groupnorm_override_shapes_are_chunked_by_the_rule():
    """... and fused only under the $ALDM_GN_FUSED_MAX the GPU test's child process sets."""
    from audioldm2_amd import ops
    for B, P, C in nf.GN_OVERRIDE_SHAPES:
        assert ops.groupnorm_plan(B, P, C)["form"] == "chunked"
        assert P <= 1024 and P * C <= nf.GN_OVERRIDE_FUSED_MAX and ops.groupnorm_plan(B, P, C)["groups_per_block"] <= 4


def test_layernorm_table_reaches_every_instantiation():
    """layernorm_launch: value slots per lane nv = ceil(C / 256) -> instantiations (1, 2 : one row per wave), (3, 4 : two rows per
    wave), (5 .. 8 : one row)."""
    nv = lambda C: (C // 4 + 63) // 64
    inst = lambda C: 1 if nv(C) <= 1 else 2 if nv(C) <= 2 else 4 if nv(C) <= 4 else 8
    assert {inst(C) for C in nf.LN_C} == {1, 2, 4, 8}
    assert [inst(C) for C in (256, 260, 512, 516, 1024, 1028)] == [1, 2, 2, 4, 4, 8]       # both sides of every threshold
    assert any((C // 4) % 64 for C in nf.LN_C) and any(C % 32 for C in nf.LN_C) and max(nf.LN_C) == 2048
    assert any(M % 2 for M in nf.LN_M) and 1 in nf.LN_M          # odd row counts: the two-rows-per-wave form clamps and breaks
    assert all(nv(C) <= 2 for C in nf.LN_ENV_C) and {nv(C) for C in nf.LN_ENV_C} == {1, 2}   # $ALDM_LN_R acts for C <= 512 only
    assert any(M % r for M in nf.LN_ENV_M for r in nf.LN_ENV_R) and 1 in nf.LN_ENV_M


def test_softmax_refuses_a_row_beyond_the_lds_stage():
    """Validation happens before any launch: the three row-softmax entry points accept 15360 floats (60 KiB) and refuse 15361 with
    the library's message."""
    from audioldm2_amd import lib
    l = lib.load()
    p = ctypes.c_void_p(4096)   # never dereferenced: validation fails first
    assert max(nf.SOFTMAX_N) * 4 == 60 * 1024 and nf.SOFTMAX_N_REFUSED == max(nf.SOFTMAX_N) + 1
    N = nf.SOFTMAX_N_REFUSED
    for call in (lambda n: l.aldm_softmax_rows(p, p, 1, n, 1.0, None), lambda n: l.aldm_softmax_rows_masked(p, p, 1, 1, 1, n, 1.0, p, 0, None),
                 lambda n: l.aldm_softmax_rows_bias(p, p, 1, 1, 1, n, 1.0, p, p, None)):
        rc = call(N)
        assert rc != 0
        with pytest.raises(RuntimeError, match=nf.SOFTMAX_REFUSAL):
            lib.check(rc, "softmax")
