"""The hand-built SearchByProjection scenes (tests/projection_cases.py) on the CPU: projection_ref gives the
prescribed reason and match for every named point, the oracle equals projection_ref bit for bit, and the
structural claims of each group (which path of the kernels it is meant to reach) hold on the reference's
diagnostics."""
from __future__ import annotations

import numpy as np
import pytest

import projection_cases as cases
import projection_ref as ref

f32 = np.float32


reference = cases.reference


@pytest.mark.parametrize("name", list(cases.GROUPS))
def test_group(pkg, oracle, name):
    g, C, X, r = reference(pkg, name)
    assert len(r.points) == len(g.names) == len(g.expected)
    for i, (p, nm, ex) in enumerate(zip(r.points, g.names, g.expected)):
        assert p.reason == ex, f"{name}: {nm}: {ref.REASONS[p.reason]}, prescribed {ref.REASONS[ex]} ({p})"
        if i in g.expected_match:
            assert p.match == g.expected_match[i], f"{name}: {nm}: keypoint {p.match}, prescribed {g.expected_match[i]}"
        if i in g.intended_uv and p.reason not in (ref.NOT_VALID, ref.BEHIND):
            u, v = g.intended_uv[i]
            assert p.u.view(np.uint32) == f32(u).view(np.uint32) and p.v.view(np.uint32) == f32(v).view(np.uint32), \
                f"{name}: {nm}: projected to ({p.u!r}, {p.v!r}), intended ({u!r}, {v!r})"
    pr = g.params
    if g.kind == "frame":
        n, m = oracle.search_by_projection_frame(C, X, pr["th"], pr["mono"], pr["check_ori"])
    else:
        n, m = oracle.search_by_projection_local(C, X, pr["th"], pr["far"], pr["th_far"], pr["ratio"], pr["taken"])
    bad = np.flatnonzero(m != r.assign)
    assert n == r.n and len(bad) == 0, f"{name}: oracle {n} vs reference {r.n}; keypoints {bad[:8]}: {m[bad[:8]]} vs {r.assign[bad[:8]]}"
    # the count: every match, minus the rotation filter's removals
    assert r.n == sum(p.reason == ref.MATCHED for p in r.points)
    c = g.claims
    if "rounds_needed" in c:
        assert r.rounds_needed >= c["rounds_needed"], r.rounds_needed
    if "affected_gt" in c:
        assert r.n_affected > c["affected_gt"], r.n_affected
    if "n_cur" in c:
        assert C.N == c["n_cur"]
    if c.get("motif_last"):   # the contested keypoints have the frame's highest indices
        contested = [p.match for p in r.points if p.claimed_before and p.match >= 0]
        assert contested and min(contested) >= c["n_cur"] - cases.MOTIF
    for i, k in c.get("n_cands", {}).items():
        assert len(r.points[i].cands) == k, (g.names[i], len(r.points[i].cands))
    for i, k in c.get("winner_pos_gt", {}).items():
        pos = [j for j, _ in r.points[i].cands].index(g.expected_match[i])
        assert pos > k, (g.names[i], pos)
    for i, (claimed, rank) in c.get("exhaustion", {}).items():
        p = r.points[i]
        assert p.claimed_before >= 8 and p.claimed_before == claimed and p.rank == rank, (g.names[i], p)
    for i, rank2 in c.get("second_rank", {}).items():
        p = r.points[i]
        assert p.rank2 == rank2 and p.n_usable > 8 and p.claimed_before == 7, (g.names[i], p)
    if c.get("hist") is not None:
        assert r.hist == c["hist"] and tuple(r.kept_bins) == tuple(c["kept"]), (r.hist, r.kept_bins)
    for i, b in c.get("bins", {}).items():
        assert r.points[i].bin == b, (g.names[i], r.points[i].bin)
    for k in c.get("ends_unassigned", []):
        assert r.assign[k] == -1


def test_structure_of_the_scenes(pkg):
    """Claims that are about the scenes themselves."""
    # half cells: the float products are exactly k + 0.5, and the reference's cells are C round's
    g, C, _, r = reference(pkg, "frame_grid")
    gx, gy = ref.grid_products(C)
    off, order = ref.build_grid(C)
    cell_of = np.full(C.N, -1)
    for c in range(ref.COLS * ref.ROWS):
        cell_of[order[off[c]:off[c + 1]]] = c
    evens = 0
    for j, (axis, prod) in g.claims["half_cells"].items():
        got = gx[j] if axis == "x" else gy[j]
        assert got == prod and float(prod) % 1.0 == 0.5, (j, got)
        k = int(np.floor(float(prod))) + 1
        assert (cell_of[j] // ref.ROWS if axis == "x" else cell_of[j] % ref.ROWS) == k
        evens += int(np.floor(float(prod))) % 2 == 0
    assert 0 < evens < len(g.claims["half_cells"])   # even and odd floors
    assert all(cell_of[j] == -1 for j in g.claims["outside"])
    # the window walk: more than 64 cells
    g, C, _, r = reference(pkg, "frame_window_walk")
    for p in r.points:
        x0, x1, y0, y1 = ref.window_cells(C, p.u, p.v, p.radius)
        assert (x1 - x0 + 1) * (y1 - y0 + 1) > g.claims["cells_gt"]
        xs = sorted({cell_of_x for cell_of_x in (int(ref.roundf(f32(f32(C.mvKeysUn["x"][j]) * f32(0.1)))) for j, _ in p.cands)})
        assert any(b - a > 1 for a, b in zip(xs, xs[1:]))   # empty columns between occupied ones
    # the tie whose winner has the higher index
    g, _, _, _ = reference(pkg, "frame_distance")
    late, first = g.claims["late_lower_index"]
    assert late < first
    # the rotation half bin: rot * (1 / 30) is exactly 4.5
    rot = cases.rot_for_half(4)
    assert f32(rot * f32(f32(1) / f32(30))) == f32(4.5)
    # the 0.1f cuts sit exactly on the counts used
    assert f32(0.1) * f32(20) == f32(2) and f32(0.1) * f32(10) == f32(1)
    # ratio products
    assert f32(0.9) * f32(50) == f32(45) and 0.9 * 50 >= 45 > float(f32(0.9)) * 50 and f32(0.8) * f32(50) == f32(40) and f32(0.6) * f32(50) > f32(30)


def test_rotation_counts(pkg):
    """An assignment in a cut bin takes the count down by one each, the keypoint to -1."""
    on = reference(pkg, "frame_rotation")[3]
    off = reference(pkg, "frame_rotation_off")[3]
    removed = sum(p.reason == ref.REMOVED for p in on.points)
    assert removed >= 4 and off.n - on.n == removed
    assert reference(pkg, "frame_rotation_third")[0].claims["third_kept"]
    assert reference(pkg, "frame_rotation_third")[3].kept_bins == (1, 2, 3)
    assert reference(pkg, "frame_rotation_third_cut")[3].kept_bins == (1, 2, -1)
    assert reference(pkg, "frame_rotation_second_cut")[3].kept_bins == (1, -1, -1)
