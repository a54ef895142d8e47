"""Ragged planes of the small-map F(3x3,3x3) layers (roi_c1: 7x7 -> 5x5 outputs as 2x2 tiles): plane index 4 -- the point at
infinity -- feeds only the third output of a tile, so a tile whose third output row / column lies outside the map never reads the
planes (4, .) / (., 4).  Plane (i, j) therefore has its own tile grid (tiles_h - [i == 4 and Ho % 3 != 0]) x
(tiles_w - [j == 4 and Wo % 3 != 0]) and the plane GEMM computes 81 instead of 100 (plane, tile) products per ROI.  Checked here
without a GPU: (1) the rule against the exact output matrix, (2) the plans' per-plane column counts, (3) the tile decode the kernel's
producer and consumer share, and the segment lists of the persistent grid, replayed on the host."""
import importlib.util
import os

import numpy as np
import pytest

_spec = importlib.util.spec_from_file_location(
    "wino_matrices", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "wino_matrices.py"))
wm = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(wm)


def _cdiv(a, b):
    return (a + b - 1) // b


def _grid(i, j, Ho, Wo):
    """The plane's own tile grid by the rule."""
    return _cdiv(Ho, 3) - (1 if i == 4 and Ho % 3 else 0), _cdiv(Wo, 3) - (1 if j == 4 and Wo % 3 else 0)


# (6x6 and 7x7: the rule gives 100 -- nothing dropped on exactly tiled maps -- and 16 x 9 + 4 x 6 + 4 x 6 + 4 = 196 of 225)
@pytest.mark.parametrize("Ho,Wo,kept", [(5, 5, 81), (5, 3, 45), (8, 4, 126), (6, 6, 100), (7, 7, 196)])
def test_dropped_pairs_have_zero_coefficients_and_kept_pairs_do_not(Ho, Wo, kept):
    AT, _, _ = wm.matrices(3, [0, 1, -1, 2])
    assert AT == [[1, 1, 1, 1, 0], [0, 1, -1, 2, 0], [0, 1, 1, 4, 1]]          # the device's output transform (winograd.hip)
    th, tw = _cdiv(Ho, 3), _cdiv(Wo, 3)
    n_kept = 0
    for i in range(5):
        for j in range(5):
            gh, gw = _grid(i, j, Ho, Wo)
            for ty in range(th):
                for tx in range(tw):
                    # coefficient of plane (i, j) in output (a, b) of the tile: AT[a][i] AT[b][j]; in-map outputs only
                    used = any(AT[a][i] != 0 and AT[b][j] != 0
                               for a in range(3) for b in range(3) if 3 * ty + a < Ho and 3 * tx + b < Wo)
                    live = ty < gh and tx < gw
                    assert used == live, (i, j, ty, tx)
                    n_kept += live
    assert n_kept == kept
    assert n_kept == sum(_grid(i, j, Ho, Wo)[0] * _grid(i, j, Ho, Wo)[1] for i in range(5) for j in range(5))


@pytest.fixture(scope="module")
def hip():
    from mscnn_amd import hipapi
    hipapi.lib()          # (planning needs no device)

    class Plan(hipapi.ConvPlan):          # plans only: no packed-weight / workspace buffers
        def _alloc(self):
            pass

        @property
        def ws_bytes(self):
            return hipapi.lib().mscnn_conv2d_workspace_bytes(self._p)

        @property
        def packed_bytes(self):
            return hipapi.lib().mscnn_conv2d_packed_weight_bytes(self._p)
    return hipapi, Plan


def _plan(hip_plan, R, Cin, H, W, Cout, pad, algo=None, tune_variant=0, tune_flags=0):
    hip, PlanOnly = hip_plan
    return PlanOnly(R, Cin, H, W, Cout, 3, 3, (pad, pad), relu=True, device="cpu", algo=hip.ALGO_WINO_F3 if algo is None else algo,
                        tune_variant=tune_variant, tune_flags=tune_flags)


def _want_cols(R, Ho, Wo):
    return [R * _grid(i, j, Ho, Wo)[0] * _grid(i, j, Ho, Wo)[1] for i in range(5) for j in range(5)]


BIT17, BIT7 = 1 << 17, 1 << 7
ROI_C1 = [(R, 1024, 7, 7, 512, 0) for R in (8, 9, 37, 696, 2000)]
OTHER = [(37, 32, 7, 5, 64, 0), (130, 32, 8, 4, 64, 1), (9, 32, 8, 8, 64, 2)]      # (the wgemm kernel needs Cout % 32 == 0; pad 2: a 10 x 10 output)


@pytest.mark.parametrize("case", ROI_C1 + OTHER)
def test_plane_columns_of_ragged_plans(hip, case):
    R, Cin, H, W, Cout, pad = case
    Ho, Wo = H + 2 * pad - 2, W + 2 * pad - 2
    p = _plan(hip, *case)
    assert p.kernel == "winograd_f3x3_3x3"
    cols = p.plane_columns()
    assert cols == _want_cols(R, Ho, Wo)
    if (H, W) == (7, 7):
        assert sorted(cols) == [R] + [2 * R] * 8 + [4 * R] * 16 and sum(cols) == 81 * R
        assert cols[24] == R and cols[4] == cols[9] == cols[20] == cols[23] == 2 * R
    assert p.executed_flops == 2.0 * Cout * Cin * sum(cols)
    uniform = _plan(hip, *case, tune_flags=BIT17)
    T = R * _cdiv(Ho, 3) * _cdiv(Wo, 3)
    assert uniform.plane_columns() == [T] * 25 and uniform.executed_flops == 2.0 * Cout * Cin * 25 * T
    assert p.ws_bytes == uniform.ws_bytes and p.packed_bytes == uniform.packed_bytes
    assert _plan(hip, *case, tune_flags=BIT7).plane_columns() == [T] * 25         # the igemm fall-back keeps uniform planes
    # the ROI count changes per frame: plan_set_batch recomputes the columns with the GEMM plan
    p.set_batch(R + 5)
    assert p.plane_columns() == _want_cols(R + 5, Ho, Wo)


def test_plane_columns_stay_uniform_elsewhere(hip):
    p = _plan(hip, 20, 64, 6, 6, 48, 1)                                         # 6 x 6 outputs: whole tiles
    assert p.kernel == "winograd_f3x3_3x3" and p.plane_columns() == [20 * 4] * 25
    f4 = _plan(hip, 1, 64, 24, 40, 64, 1, algo=hip[0].ALGO_WINO_F4)                # F(4x4,3x3): 36 planes
    assert f4.kernel == "winograd_f4x4_3x3" and f4.plane_columns() == [6 * 10] * 36
    f3 = _plan(hip, 1, 64, 23, 40, 64, 1)                                       # a whole map in F(3x3,3x3): 23 % 3 != 0, still uniform
    assert f3.kernel == "winograd_f3x3_3x3" and f3.plane_columns() == [8 * 14] * 25
    assert _plan(hip, 4, 16, 9, 9, 8, 0, algo=hip[0].ALGO_DIRECT).plane_columns() == []


TILE = {1: (256, 128), 2: (128, 256), 3: (128, 128), 4: (256, 96), 5: (256, 160)}


@pytest.mark.parametrize("variant", [0, 1, 2, 3, 4, 5])
@pytest.mark.parametrize("case", ROI_C1 + OTHER + [(20, 64, 6, 6, 64, 1)])
def test_tile_decode_and_segments_cover_every_unit_once(hip, case, variant):
    """The decode t -> (plane, column tile, row tile) the kernel's producer and consumer share, through the host replay of the
    persistent grid's segment cursors: with whole tiles, slot s takes t = s, s + G, ... -- so the replay enumerates t; every
    (p, nt < NT_p, mt < MT) must come exactly once, in increasing t.  Then the split (forced, and the plan's own choice): the
    segments of the G slots cover every (tile, chunk) exactly once, and the parts of a split tile lie, in k order, in the next
    slots that have remainder work."""
    R, Cin, H, W, Cout, pad = case
    for flags in (0, BIT17):
        cols = _plan(hip, *case, tune_flags=flags).plane_columns()
        for sched in (512, 256, 0):
            if sched == 0 and variant == 0:
                tv = 0
            else:
                tv = 300 + variant + sched
            p = _plan(hip, *case, tune_variant=tv, tune_flags=flags)
            got = p.debug_wgemm_schedule()
            assert got is not None
            info, rows = got
            assert info["ragged"] == (1 if cols != [max(cols)] * 25 and flags == 0 else 0)
            BN, MT, KI, G = info["BN"], info["MT"], info["KI"], info["G"]
            if variant:
                assert (BN == TILE[variant][1]) and MT == _cdiv(Cout, TILE[variant][0])
            assert G == 256 and KI == Cin // 32
            want = [(pl, nt, mt) for pl in range(25) for nt in range(_cdiv(cols[pl], BN)) for mt in range(MT)]
            assert info["tiles"] == len(want)
            if sched == 512:
                assert (rows[:, 6] == -1).all() and (rows[:, 4] == 0).all() and (rows[:, 5] == KI).all()
                # row r of slot s is tile s + r G
                t = np.empty(len(rows), dtype=np.int64)
                seen = {}
                for n, s in enumerate(rows[:, 0]):
                    t[n] = s + seen.get(int(s), 0) * G
                    seen[int(s)] = seen.get(int(s), 0) + 1
                order = np.argsort(t, kind="stable")
                assert (t[order] == np.arange(len(want))).all()
                assert [tuple(r) for r in rows[order, 1:4]] == want
            # every (tile, chunk) exactly once
            index = {u: n for n, u in enumerate(want)}
            cover = np.zeros((len(want), KI), dtype=np.int32)
            for slot, pl, nt, mt, k0, k1, part in rows:
                assert 0 <= k0 < k1 <= KI and (pl, nt, mt) in index
                cover[index[(pl, nt, mt)], k0:k1] += 1
                assert (part == -1) == (k0 == 0 and k1 == KI)
            assert (cover == 1).all()
            # the hand-off the finisher relies on: the parts of a split tile, in k order, lie in increasing slots, the first one
            # (k0 == 0, the finisher) lowest; the slots between two of them hold no remainder work at all (the finisher skips empty
            # ranges and adds slot + 1, slot + 2, ... in that order); a slot publishes at most one slab
            partial = rows[rows[:, 6] >= 0]
            slots_with_partials = set(int(s) for s in partial[:, 0])
            for s in slots_with_partials:
                assert (partial[partial[:, 0] == s][:, 4] > 0).sum() <= 1
            tiles_split = {}
            for slot, pl, nt, mt, k0, k1, part in partial:
                tiles_split.setdefault((int(pl), int(nt), int(mt)), []).append((int(k0), int(k1), int(slot)))
            for parts in tiles_split.values():
                parts.sort()
                assert parts[0][0] == 0 and parts[-1][1] == KI and len(parts) >= 2
                for (a0, a1, sa), (b0, b1, sb) in zip(parts, parts[1:]):
                    assert a1 == b0 and sa < sb
                    assert not any(sa < s < sb for s in slots_with_partials)
            # the whole-tile replay of the same plan (what a launch does after a reported hand-off time-out)
            info_w, rows_w = p.debug_wgemm_schedule(whole_tiles=True)
            assert sorted(tuple(r) for r in rows_w[:, 1:4]) == want and (rows_w[:, 6] == -1).all()
