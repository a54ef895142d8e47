"""The convolution plan classes the deploy nets select against the classes the small GPU cases exercise (tests/conv_classes.py), and
two host-side sweeps of the planner: a re-planned plan equals a fresh one in every getter, and the replay of the plane GEMM's schedule
covers every (plane, column tile, row tile) k-range exactly once.  Planning needs no device."""
import numpy as np
import pytest

import conv_classes as cc
from mscnn_amd import hipapi


@pytest.fixture(scope="module")
def census():
    return cc.census()


@pytest.mark.parametrize("row", cc.CASES, ids=[r["id"] for r in cc.CASES])
def test_row_plans_to_the_class_it_names(row):
    want = cc.class_of_row(row)
    got = cc.plan_class(row["desc"])
    assert got == want, f"{row['id']} (stands for {row['layer']}): {cc.diff(got, want)}"
    # the second forward's batch (another N of the same class)
    got2 = cc.plan_class(dict(row["desc"], N=row["N2"]))
    assert row["N2"] != row["desc"]["N"] and got2 == want, f"{row['id']} at N2 = {row['N2']}: {cc.diff(got2, want)}"


@pytest.mark.parametrize("row", cc.CASES, ids=[r["id"] for r in cc.CASES])
def test_row_is_within_the_size_cap(row):
    for N in (row["desc"]["N"], row["N2"]):
        d = dict(row["desc"], N=N)
        p = cc.make_plan(d)
        n_, co, ho, wo = p.out_shape()
        tensors = [N * d["Cin"] * d["H"] * d["W"] * 4, n_ * co * ho * wo * 4, co * d["Cin"] * d["Kh"] * d["Kw"] * 4]
        assert max(tensors) <= cc.MAX_TENSOR_BYTES, tensors
        assert max(p.ws_bytes, p.packed_bytes) <= cc.MAX_SCRATCH_BYTES, (p.ws_bytes, p.packed_bytes)
        assert p.flops <= cc.MAX_FLOPS, p.flops


def test_ids_are_unique_and_rows_name_a_deploy_layer(census):
    ids = [r["id"] for r in cc.CASES]
    assert len(set(ids)) == len(ids)
    for r in cc.CASES:
        cls = cc.class_of_row(r)
        assert cls in census, f"{r['id']}: no deploy layer selects {cc.brief(cls)} any more -- drop the row or move it to the class it was written for"
        assert any(f"{m}:{l}" == r["layer"] for m, l, *_ in census[cls]), \
            f"{r['id']} stands for {r['layer']}, which does not select its class; layers that do: {sorted(set(f'{m}:{l}' for m, l, *_ in census[cls]))[:6]}"


def test_every_class_a_deploy_layer_selects_has_a_row(census):
    covered = {cc.class_of_row(r) for r in cc.CASES}
    orphans = [c for c in census if c not in covered and c not in cc.UNREACHED]
    lines = [f"{cc.brief(c)}   <- {len(census[c])} layers, e.g. {census[c][0][:4]}" for c in sorted(orphans)]
    assert not orphans, "plan classes without a small GPU case:\n" + "\n".join(lines)


def test_unreached_is_small_and_holds_no_benchmark_class(census):
    for c, why in cc.UNREACHED.items():
        assert c in census and why, f"UNREACHED names a class no deploy layer selects: {cc.brief(c)}"
        assert c not in {cc.class_of_row(r) for r in cc.CASES}, f"UNREACHED class has a row: {cc.brief(c)}"
        bench = [e[:4] for e in census[c] if e[0] in cc.BENCH_MODELS and e[2] in ("AUTO", "DIRECT")]
        assert not bench, f"a class the benchmark's nets select is UNREACHED: {cc.brief(c)} <- {bench[:3]}"
    assert len(cc.UNREACHED) * 10 <= len(census), (len(cc.UNREACHED), len(census))


def test_census_sees_the_classes_the_issue_counted(census):
    """Classes that appear only at full size: they must be in the census (else the walk lost layers), whatever covers them."""
    d = [cc.as_dict(c) for c in census]
    assert any(c["wino_m"] == 4 and c["wg_bn"] == 160 and c["can_pool"] for c in d)
    assert any(c["wino_m"] == 4 and c["wg_bn"] == 128 and c["wg_bm"] == 256 and c["can_pool"] for c in d)
    assert any(c["wino_m"] == 3 and c["wg_ragged"] and c["wg_bn"] == 160 for c in d)
    assert any(c["wino_m"] == 3 and c["wg_ragged"] and not c["wg_split"] for c in d)
    assert any(c["wino_m"] == 3 and c["wg_bn"] == 96 and c["can_pool"] for c in d)
    assert len(census) >= 100


# ---- re-planning -------------------------------------------------------------------------------------------------------------------
def _getters(p):
    sched = p.debug_wgemm_schedule()
    L = hipapi.lib()
    return {"kernel": p.kernel, "dtype": p.dtype, "flops": p.flops, "executed_flops": p.executed_flops, "plane_columns": p.plane_columns(),
            "ws_bytes": p.ws_bytes, "packed_bytes": p.packed_bytes, "weight_layout": L.mscnn_conv2d_plan_weight_layout(p._p),
            "can_pool": p.can_pool, "can_pool_only": p.can_pool_only, "publishes_amax": p.publishes_amax, "class": tuple(p.plan_class().values()),
            "wgemm": None if sched is None else (sched[0], sched[1].tobytes())}


REPLAN_LAYERS = [   # Cin, H, W, Cout, Kh, Kw, pad
    (3, 480, 640, 64, 3, 3, (1, 1)), (64, 480, 640, 64, 3, 3, (1, 1)), (64, 240, 320, 128, 3, 3, (1, 1)), (128, 120, 160, 256, 3, 3, (1, 1)),
    (256, 60, 80, 512, 3, 3, (1, 1)), (512, 30, 40, 512, 3, 3, (1, 1)), (512, 15, 20, 512, 3, 3, (1, 1)), (512, 18, 60, 512, 3, 3, (1, 1)),
    (1024, 7, 7, 512, 3, 3, (0, 0)), (1024, 7, 5, 512, 3, 3, (0, 0)), (1024, 8, 4, 512, 3, 3, (1, 1)), (32, 8, 8, 64, 3, 3, (2, 2)),
    (512, 72, 240, 9, 7, 7, (3, 3)), (512, 36, 120, 9, 5, 5, (2, 2)), (512, 15, 20, 6, 5, 3, (2, 1)), (512, 64, 64, 6, 1, 1, (0, 0)),
]
REPLAN_NS = [0, 1, 2, 7, 8, 9, 37, 300, 2000]      # across 0, the ROI layers' 7 / 8, and the tile-count thresholds of the layers above


@pytest.mark.parametrize("algo", ["AUTO", "DIRECT", "WINO_F2", "WINO_F3", "F16", "WINO_F3_X3", "WINO_F4"])
def test_replanned_plan_equals_a_fresh_one_in_every_getter(algo):
    code = getattr(hipapi, "ALGO_" + algo)
    bad = []
    for (Cin, H, W, Cout, Kh, Kw, pad) in REPLAN_LAYERS:
        fresh = {}
        for N in REPLAN_NS:
            fresh[N] = _getters(cc.PlanOnly(N, Cin, H, W, Cout, Kh, Kw, pad, relu=True, device="cpu", algo=code))
        for a in REPLAN_NS:
            p = cc.PlanOnly(a, Cin, H, W, Cout, Kh, Kw, pad, relu=True, device="cpu", algo=code)
            for b in REPLAN_NS:
                if a == b:
                    continue
                p.set_batch(b)
                got = _getters(p)
                if got != fresh[b]:
                    bad.append(((Cin, H, W, Cout, Kh, Kw, pad), a, b, [k for k in got if got[k] != fresh[b][k]]))
                p.set_batch(a)
                if _getters(p) != fresh[a]:
                    bad.append(((Cin, H, W, Cout, Kh, Kw, pad), f"{a} -> {b} ->", a, "back"))
    assert not bad, bad[:10]


# ---- schedule replay -----------------------------------------------------------------------------------------------------------------
def _schedule_holes(p):
    """0 where the plan's replay covers every (tile, chunk) exactly once; else a description."""
    got = p.debug_wgemm_schedule()
    assert got is not None
    info, rows = got
    MT, KI, BN = info["MT"], info["KI"], info["BN"]
    cols = np.asarray(p.plane_columns())
    nt = (cols + BN - 1) // BN if info["ragged"] else np.full(len(cols), (cols.max() + BN - 1) // BN)
    off = np.concatenate([[0], np.cumsum(nt)])
    if info["tiles"] != MT * off[-1]:
        return f"tiles {info['tiles']} != {MT * off[-1]}"
    pl, cnt, mt, k0, k1, part = (rows[:, i].astype(np.int64) for i in range(1, 7))
    if not ((0 <= k0) & (k0 < k1) & (k1 <= KI) & (cnt < nt[pl]) & (mt < MT) & ((part == -1) == ((k0 == 0) & (k1 == KI)))).all():
        return "a segment outside its plane's tiles or k range"
    t = (off[pl] + cnt) * MT + mt
    delta = np.zeros((info["tiles"], KI + 1), dtype=np.int64)
    np.add.at(delta, (t, k0), 1)
    np.add.at(delta, (t, k1), -1)
    cover = np.cumsum(delta, axis=1)[:, :KI]
    if not (cover == 1).all():
        return f"{int((cover != 1).sum())} (tile, chunk) units not covered exactly once"
    return 0


def test_wgemm_schedule_replay_covers_every_k_range_exactly_once():
    rng = np.random.default_rng(20240611)
    kinds = set()
    checked = 0
    for trial in range(4000):
        f4 = bool(trial % 2)
        variant = int(rng.integers(0, 6))
        sched = int(rng.choice([0, 256, 512]))
        tv = 300 + variant + sched if variant + sched else 0
        Cin, Cout = int(rng.choice([32, 64, 96, 256, 1024])), int(rng.choice([32, 64, 160, 256, 512]))
        if f4 or trial % 4 == 0:      # whole maps
            N, H, W, pad = int(rng.integers(1, 4)), int(rng.integers(6, 90)), int(rng.integers(6, 200)), 1
            flags = 0
        else:                         # small maps: ragged planes, or the same shape with uniform ones
            N, (H, W, pad) = int(rng.integers(8, 2100)), [(7, 7, 0), (7, 5, 0), (8, 4, 1), (8, 8, 2), (6, 6, 1)][int(rng.integers(0, 5))]
            flags = (1 << 17) if trial % 8 == 6 else 0
        p = cc.PlanOnly(N, Cin, H, W, Cout, 3, 3, (pad, pad), relu=True, device="cpu", algo=hipapi.ALGO_WINO_F4 if f4 else hipapi.ALGO_WINO_F3,
                        tune_variant=tv, tune_flags=flags)
        if p.debug_wgemm_schedule() is None:
            continue          # (beyond the 32-bit windows: the plan keeps the igemm GEMM)
        c = p.plan_class()
        kinds.add((c["wino_m"], c["wg_bn"], c["wg_split"], bool(c["wg_ragged"])))
        holes = _schedule_holes(p)
        checked += 1
        assert holes == 0, ((N, Cin, H, W, Cout, pad, tv, flags), holes)
        info_w, rows_w = p.debug_wgemm_schedule(whole_tiles=True)
        assert (rows_w[:, 6] == -1).all() and len(rows_w) == info_w["tiles"]
    assert checked >= 3000, checked
    # the sample holds every kind of plan: both forms, every tile width, split and whole, ragged and uniform
    for m in (3, 4):
        for bn in (96, 128, 160, 256):
            for split in (0, 1):
                assert (m, bn, split, False) in kinds, (m, bn, split)
    assert {(3, bn, s, True) for bn in (96, 128, 160, 256) for s in (0, 1)} <= kinds


def test_the_committed_listing_is_current():
    import os
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "CONV_CLASSES.md")
    assert open(path).read() == cc.listing(), "tests/CONV_CLASSES.md is stale: python tests/conv_classes.py > tests/CONV_CLASSES.md"
