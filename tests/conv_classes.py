"""Plan classes of the convolution kernels: which kernel build runs a layer, and in which mode (mscnn_debug_conv_plan_class).

census()  -- every Convolution layer of every deploy net of mscnn_amd.zoo.MODELS at its shipped input size, planned on the host under
             the algos a net can run: class -> the layers that select it.
CASES     -- small GPU cases, one or more per class: the desc (tune knobs included), the class it is meant to hit written out, and the
             deploy layer it stands for.  tests/test_conv_class_census_cpu.py holds the two together; tests/test_gpu_conv_classes.py
             runs CASES against a float64 reference.
Plans only: nothing here needs a device."""
import functools
import os
import sys

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if _ROOT not in sys.path:      # (also runs as a script: python tests/conv_classes.py prints the listing)
    sys.path.insert(0, _ROOT)

from mscnn_amd import hipapi      # noqa: E402

ALGOS = {"AUTO": hipapi.ALGO_AUTO, "DIRECT": hipapi.ALGO_DIRECT, "F16": hipapi.ALGO_F16, "WINO_F3_X3": hipapi.ALGO_WINO_F3_X3,
         "WINO_F2": hipapi.ALGO_WINO_F2, "WINO_F3": hipapi.ALGO_WINO_F3, "WINO_F4": hipapi.ALGO_WINO_F4}
NET_ALGOS = ("AUTO", "DIRECT", "F16", "WINO_F3_X3")   # what a net runs: its default, the numerical fall-back, the two reduced-operand modes
BATCHES = (1, 2, 4, 8)                                # bench.py's default and the README's --batch lines
ROI_COUNTS = (1, 7, 8, 37, 300, 676, 2000)            # layers fed by ROIs: the count changes per frame
BENCH_MODELS = ("kitti_car/mscnn-7s-576", "caltech/mscnn-7s-480")


class PlanOnly(hipapi.ConvPlan):
    """A plan without packed-weight / workspace buffers (planning needs no device)."""

    def _alloc(self):
        pass

    @property
    def ws_bytes(self):
        return hipapi.lib().mscnn_conv2d_workspace_bytes(self._p)

    @property
    def packed_bytes(self):
        return hipapi.lib().mscnn_conv2d_packed_weight_bytes(self._p)


def make_plan(desc, cls=PlanOnly, device="cpu"):
    """desc: dict(N, Cin, H, W, Cout, Kh, Kw, pad=(ph, pw), algo="AUTO", tune_variant=0, tune_grid=0, tune_flags=0[, relu])."""
    return cls(desc["N"], desc["Cin"], desc["H"], desc["W"], desc["Cout"], desc["Kh"], desc["Kw"], tuple(desc.get("pad", (0, 0))),
               tuple(desc.get("stride", (1, 1))), desc.get("group", 1), relu=desc.get("relu", True), device=device,
               algo=ALGOS[desc.get("algo", "AUTO")], tune_variant=desc.get("tune_variant", 0), tune_grid=desc.get("tune_grid", 0),
               tune_flags=desc.get("tune_flags", 0))


@functools.lru_cache(maxsize=None)
def fields():
    return tuple(make_plan(dict(N=1, Cin=8, H=8, W=8, Cout=8, Kh=3, Kw=3)).plan_class())


def plan_class(desc):
    """The class of the plan `desc` makes, as a tuple of ints in the order of fields()."""
    return tuple(make_plan(desc).plan_class().values())


def as_dict(cls):
    return dict(zip(fields(), cls))


def brief(cls):
    """The non-zero fields of a class, for messages and the summary."""
    return ", ".join(f"{k}={v}" for k, v in as_dict(cls).items() if v)


def diff(got, want):
    return ", ".join(f"{k}: planned {g}, table says {w}" for k, g, w in zip(fields(), got, want) if g != w) or "(equal)"


def _conv_layers(model, batch):
    """(layer name, desc without algo, fed by ROIs?) of every Convolution layer of the net, built on the host."""
    from mscnn_amd import net as mnet, zoo
    from oracle import pynet      # (test infrastructure: the parser of the runtime's layer text)
    n = mnet.Net(prototxt_text=zoo.prototxt(model, batch=batch), device=-1)
    roi_blobs, out = set(), []
    for i, typ in enumerate(n.layer_types):
        bottoms = n.layer_bottoms(i)
        if typ.startswith("ROI") or any(b in roi_blobs for b in bottoms):
            roi_blobs.update(n.layer_tops(i))
        if typ != "Convolution":
            continue
        kh, kw, ph, pw, sh, sw, g = pynet._conv_geom(pynet.parse_param_text(n.layer_param_text(i))["convolution_param"][0])
        N, Cin, H, W = n.blob_shape(bottoms[0])
        wshape = n.param_shapes(i)[0]
        assert wshape[1] * g == Cin and (wshape[2], wshape[3]) == (kh, kw), (model, n.layer_names[i], wshape)
        out.append((n.layer_names[i], dict(N=N, Cin=Cin, H=H, W=W, Cout=wshape[0], Kh=kh, Kw=kw, pad=(ph, pw), stride=(sh, sw), group=g),
                    bottoms[0] in roi_blobs))
    return out


@functools.lru_cache(maxsize=None)
def census():
    """class -> sorted list of (model, layer, algo, batch or 'R=<rois>', desc items) that select it."""
    from mscnn_amd import zoo
    found = {}
    for model in sorted(zoo.MODELS):
        for batch in BATCHES:
            for name, desc, roi_fed in _conv_layers(model, batch):
                if roi_fed and batch != 1:
                    continue          # (the ROI count, not the batch, is such a layer's N)
                for R in (ROI_COUNTS if roi_fed else (None,)):
                    for algo in NET_ALGOS:
                        d = dict(desc, algo=algo)
                        if R is not None:
                            d["N"] = R
                        found.setdefault(plan_class(d), []).append((model, name, algo, f"R={R}" if roi_fed else f"batch={batch}", tuple(sorted(d.items()))))
    return {c: sorted(v) for c, v in found.items()}


FIELDS = fields()


# ---- the small GPU cases ---------------------------------------------------------------------------------------------------------------
# One row per class of the census.  A row reaches its class at the smallest shape that plans to it with at least three K chunks, more
# than one column tile per plane in the plane GEMMs and more than one pixel tile in the direct kernels -- through the natural threshold
# where that fits the cap, else through the documented test knobs (tune_variant: 300 + v the wgemm tile shape, + 256 / + 512 split /
# whole; 202 the fp16 occ3 build; 402 / 403 the ring / one-launch kernels on small maps; 500 full head chunks; tune_grid: the
# persistent grid, which sets the schedule mode; tune_flags: bit 2 forces the split-fp16 Winograd form, bit 7 the nested igemm GEMM,
# bit 10 the folded-column head form) or a forcing algo (WINO_F3 / WINO_F4).  How a class was reached is not part of the class.
# N2: the batch of the second forward (set_batch on the same plan), another N of the same class.
# Caps per row: x, w and y at most 64 MiB each and MAX_FLOPS of direct-convolution work; the plan's own scratch at most 128 MiB (the
# stream-K slab area of the 256 x 160 plane GEMM alone is 256 workgroups x 160 KiB = 40 MiB, whatever the shape).
MAX_FLOPS = 20e9
MAX_TENSOR_BYTES = 64 * 2 ** 20
MAX_SCRATCH_BYTES = 128 * 2 ** 20


def _row(id, layer, desc, N2, cls):
    return dict(id=id, layer=layer, desc=desc, N2=N2, cls=cls)


def class_of_row(row):
    """The class a row names (the fields it does not write out are 0), as a tuple in the order of fields()."""
    unknown = set(row["cls"]) - set(FIELDS)
    assert not unknown, (row["id"], unknown)
    return tuple(row["cls"].get(f, 0) for f in FIELDS)


CASES = [
    _row("c000", "citypersons/cascade-mscnn-8s-1344-2x:conv1_2", dict(N=1, Cin=96, H=12, W=32, Cout=64, Kh=3, Kw=3, pad=(1, 1), algo="DIRECT", tune_grid=1), 2,
         dict(family=1, entry=2, ig_sched=1, can_pool=1, can_pool_only=1, publishes_amax=1)),
    _row("c001", "kitti_car/mscnn-7s-576:conv1_2", dict(N=1, Cin=96, H=12, W=33, Cout=64, Kh=3, Kw=3, pad=(1, 1), algo="DIRECT", tune_grid=3), 2,
         dict(family=1, entry=2, ig_sched=3, can_pool=1, can_pool_only=1, publishes_amax=1)),
    _row("c002", "kitti_car/mscnn-7s-384:conv2_1", dict(N=1, Cin=96, H=16, W=24, Cout=128, Kh=3, Kw=3, pad=(1, 1), algo="DIRECT", tune_grid=1), 2,
         dict(family=1, entry=4, ig_sched=1, can_pool=1, can_pool_only=1, publishes_amax=1)),
    _row("c003", "caltech/mscnn-7s-480:conv2_1", dict(N=1, Cin=96, H=16, W=24, Cout=128, Kh=3, Kw=3, pad=(1, 1), algo="DIRECT", tune_grid=3), 2,
         dict(family=1, entry=4, ig_sched=3, can_pool=1, can_pool_only=1, publishes_amax=1)),
    _row("c004", "caltech/mscnn-7s-480:conv2_1", dict(N=1, Cin=96, H=16, W=24, Cout=128, Kh=3, Kw=3, pad=(1, 1), algo="AUTO"), 2,
         dict(family=1, entry=4, ig_sched=4, can_pool=1, can_pool_only=1, publishes_amax=1)),
    _row("c005", "kitti_car/mscnn-7s-384:conv3_1", dict(N=1, Cin=96, H=24, W=16, Cout=160, Kh=3, Kw=3, pad=(1, 1), algo="DIRECT", tune_grid=1), 2,
         dict(family=1, entry=4, ig_mt_gt1=1, ig_sched=1, can_pool=1, can_pool_only=1, publishes_amax=1)),
    _row("c006", "caltech/mscnn-7s-480:conv3_1", dict(N=1, Cin=96, H=24, W=16, Cout=160, Kh=3, Kw=3, pad=(1, 1), algo="DIRECT", tune_grid=4), 3,
         dict(family=1, entry=4, ig_mt_gt1=1, ig_sched=3, can_pool=1, can_pool_only=1, publishes_amax=1)),
    _row("c007", "caltech/mscnn-7s-480:conv3_1", dict(N=2, Cin=96, H=12, W=16, Cout=160, Kh=3, Kw=3, pad=(1, 1), algo="AUTO"), 3,
         dict(family=1, entry=4, ig_mt_gt1=1, ig_sched=4, can_pool=1, can_pool_only=1, publishes_amax=1)),
    _row("c008", "kitti_car/mscnn-7s-576:conv5_1", dict(N=1, Cin=96, H=12, W=32, Cout=160, Kh=3, Kw=3, pad=(1, 1), algo="DIRECT", tune_grid=4), 3,
         dict(family=1, entry=5, ig_mt_gt1=1, ig_sched=3, can_pool=1, can_pool_only=1, publishes_amax=1)),
    _row("c009", "kitti_car/mscnn-7s-576:conv5_1", dict(N=1, Cin=96, H=12, W=32, Cout=160, Kh=3, Kw=3, pad=(1, 1), algo="DIRECT"), 2,
         dict(family=1, entry=5, ig_mt_gt1=1, ig_sched=4, can_pool=1, can_pool_only=1, publishes_amax=1)),
    _row("c010", "widerface/cascade-mscnn-12s-align:LFCN_1_12x12", dict(N=1, Cin=128, H=4, W=8, Cout=6, Kh=1, Kw=1, pad=(0, 0), algo="AUTO"), 2,
         dict(family=1, entry=8, ig_sched=2, publishes_amax=1)),
    _row("c011", "widerface/cascade-mscnn-12s-align:LFCN_1_12x12", dict(N=1, Cin=512, H=4, W=8, Cout=6, Kh=1, Kw=1, pad=(0, 0), algo="AUTO"), 2,
         dict(family=1, entry=8, ig_sched=4, publishes_amax=1)),
    _row("c012", "widerface/cascade-mscnn-12s-align:conv2_1", dict(N=1, Cin=96, H=24, W=16, Cout=64, Kh=3, Kw=3, pad=(1, 1), algo="F16", tune_grid=1), 2,
         dict(family=1, entry=14, dtype=1, ig_sched=1, can_pool=1, can_pool_only=1)),
    _row("c013", "widerface/cascade-mscnn-12s-align:conv2_1", dict(N=1, Cin=64, H=24, W=16, Cout=64, Kh=3, Kw=3, pad=(1, 1), algo="F16"), 2,
         dict(family=1, entry=14, dtype=1, ig_sched=2, can_pool=1, can_pool_only=1)),
    _row("c014", "caltech/mscnn-7s-480:conv2_1", dict(N=1, Cin=96, H=24, W=16, Cout=64, Kh=3, Kw=3, pad=(1, 1), algo="F16", tune_grid=2), 3,
         dict(family=1, entry=14, dtype=1, ig_sched=3, can_pool=1, can_pool_only=1)),
    _row("c015", "widerface/cascade-mscnn-12s-align:conv3_1", dict(N=1, Cin=96, H=24, W=16, Cout=160, Kh=3, Kw=3, pad=(1, 1), algo="F16", tune_grid=1), 2,
         dict(family=1, entry=14, dtype=1, ig_mt_gt1=1, ig_sched=1, can_pool=1, can_pool_only=1)),
    _row("c016", "widerface/cascade-mscnn-12s-align:conv3_1", dict(N=1, Cin=64, H=24, W=16, Cout=160, Kh=3, Kw=3, pad=(1, 1), algo="F16"), 2,
         dict(family=1, entry=14, dtype=1, ig_mt_gt1=1, ig_sched=2, can_pool=1, can_pool_only=1)),
    _row("c017", "caltech/mscnn-7s-480:conv3_1", dict(N=1, Cin=96, H=24, W=16, Cout=160, Kh=3, Kw=3, pad=(1, 1), algo="F16", tune_grid=4), 3,
         dict(family=1, entry=14, dtype=1, ig_mt_gt1=1, ig_sched=3, can_pool=1, can_pool_only=1)),
    _row("c018", "caltech/mscnn-7s-480:conv3_1", dict(N=1, Cin=96, H=24, W=16, Cout=160, Kh=3, Kw=3, pad=(1, 1), algo="F16"), 2,
         dict(family=1, entry=14, dtype=1, ig_mt_gt1=1, ig_sched=4, can_pool=1, can_pool_only=1)),
    _row("c019", "citypersons/cascade-mscnn-8s-1344-2x:conv6_1", dict(N=1, Cin=96, H=12, W=32, Cout=160, Kh=3, Kw=3, pad=(1, 1), algo="F16", tune_grid=4), 3,
         dict(family=1, entry=15, dtype=1, ig_mt_gt1=1, ig_sched=3, can_pool=1, can_pool_only=1)),
    _row("c020", "citypersons/cascade-mscnn-8s-1344-2x:conv6_1", dict(N=1, Cin=96, H=12, W=32, Cout=160, Kh=3, Kw=3, pad=(1, 1), algo="F16"), 2,
         dict(family=1, entry=15, dtype=1, ig_mt_gt1=1, ig_sched=4, can_pool=1, can_pool_only=1)),
    _row("c021", "widerface/cascade-mscnn-12s-align:conv1_2", dict(N=1, Cin=96, H=12, W=32, Cout=64, Kh=3, Kw=3, pad=(1, 1), algo="F16", tune_grid=1), 2,
         dict(family=1, entry=16, dtype=1, ig_sched=1, can_pool=1, can_pool_only=1)),
    _row("c022", "caltech/mscnn-7s-480:conv1_2", dict(N=1, Cin=96, H=12, W=33, Cout=64, Kh=3, Kw=3, pad=(1, 1), algo="F16", tune_grid=3), 2,
         dict(family=1, entry=16, dtype=1, ig_sched=3, can_pool=1, can_pool_only=1)),
    _row("c023", "citypersons/cascade-mscnn-8s-1344-2x:conv1_2", dict(N=1, Cin=96, H=32, W=128, Cout=64, Kh=3, Kw=3, pad=(1, 1), algo="WINO_F3_X3", tune_grid=1), 2,
         dict(family=1, entry=18, dtype=2, ig_sched=1, can_pool=1, can_pool_only=1, publishes_amax=1)),
    _row("c024", "caltech/mscnn-7s-480:conv1_2", dict(N=1, Cin=96, H=32, W=128, Cout=64, Kh=3, Kw=3, pad=(1, 1), algo="WINO_F3_X3", tune_grid=3), 2,
         dict(family=1, entry=18, dtype=2, ig_sched=3, can_pool=1, can_pool_only=1, publishes_amax=1)),
    _row("c025", "citypersons/cascade-mscnn-8s-1344-2x:conv2_1", dict(N=1, Cin=96, H=32, W=128, Cout=128, Kh=3, Kw=3, pad=(1, 1), algo="WINO_F3_X3", tune_grid=1), 2,
         dict(family=1, entry=18, dtype=2, ig_mt_gt1=1, ig_sched=1, can_pool=1, can_pool_only=1, publishes_amax=1)),
    _row("c026", "widerface/cascade-mscnn-12s-align:conv2_1", dict(N=1, Cin=64, H=32, W=128, Cout=128, Kh=3, Kw=3, pad=(1, 1), algo="WINO_F3_X3"), 2,
         dict(family=1, entry=18, dtype=2, ig_mt_gt1=1, ig_sched=2, can_pool=1, can_pool_only=1, publishes_amax=1)),
    _row("c027", "caltech/mscnn-7s-480:conv2_1", dict(N=1, Cin=96, H=32, W=128, Cout=128, Kh=3, Kw=3, pad=(1, 1), algo="WINO_F3_X3", tune_grid=3), 2,
         dict(family=1, entry=18, dtype=2, ig_mt_gt1=1, ig_sched=3, can_pool=1, can_pool_only=1, publishes_amax=1)),
    _row("c028", "kitti_car/mscnn-7s-384:conv2_1", dict(N=1, Cin=96, H=24, W=16, Cout=64, Kh=3, Kw=3, pad=(1, 1), algo="F16", tune_variant=202, tune_grid=1), 2,
         dict(family=1, entry=19, dtype=1, ig_sched=1, can_pool=1, can_pool_only=1)),
    _row("c029", "caltech/mscnn-7s-480:conv2_1", dict(N=1, Cin=96, H=24, W=16, Cout=64, Kh=3, Kw=3, pad=(1, 1), algo="F16", tune_variant=202, tune_grid=2), 3,
         dict(family=1, entry=19, dtype=1, ig_sched=3, can_pool=1, can_pool_only=1)),
    _row("c030", "kitti_car/mscnn-7s-384:conv3_1", dict(N=1, Cin=96, H=24, W=16, Cout=160, Kh=3, Kw=3, pad=(1, 1), algo="F16", tune_variant=202, tune_grid=1), 2,
         dict(family=1, entry=19, dtype=1, ig_mt_gt1=1, ig_sched=1, can_pool=1, can_pool_only=1)),
    _row("c031", "caltech/mscnn-7s-480:conv3_1", dict(N=1, Cin=96, H=24, W=16, Cout=160, Kh=3, Kw=3, pad=(1, 1), algo="F16", tune_variant=202, tune_grid=4), 3,
         dict(family=1, entry=19, dtype=1, ig_mt_gt1=1, ig_sched=3, can_pool=1, can_pool_only=1)),
    _row("c032", "citypersons/cascade-mscnn-8s-1344-2x:conv1_2", dict(N=1, Cin=96, H=12, W=32, Cout=64, Kh=3, Kw=3, pad=(1, 1), algo="F16", tune_variant=202, tune_grid=1), 2,
         dict(family=1, entry=21, dtype=1, ig_sched=1, can_pool=1, can_pool_only=1)),
    _row("c033", "caltech/mscnn-7s-480:conv1_2", dict(N=1, Cin=96, H=12, W=33, Cout=64, Kh=3, Kw=3, pad=(1, 1), algo="F16", tune_variant=202, tune_grid=3), 2,
         dict(family=1, entry=21, dtype=1, ig_sched=3, can_pool=1, can_pool_only=1)),
    _row("c034", "kitti_car/cascade-mscnn-7s-576-2x:roi_c1", dict(N=5, Cin=64, H=7, W=7, Cout=288, Kh=3, Kw=3, pad=(0, 0), algo="F16", tune_grid=2), 15,
         dict(family=1, entry=22, dtype=1, ig_mt_gt1=1, ig_roi=1, ig_sched=3)),
    _row("c035", "kitti_car/cascade-mscnn-7s-576-2x:roi_c1", dict(N=5, Cin=96, H=7, W=7, Cout=160, Kh=3, Kw=3, pad=(0, 0), algo="F16"), 10,
         dict(family=1, entry=22, dtype=1, ig_mt_gt1=1, ig_roi=1, ig_sched=4)),
    _row("c036", "kitti_car/cascade-mscnn-7s-576-2x:roi_c1", dict(N=1, Cin=64, H=7, W=7, Cout=288, Kh=3, Kw=3, pad=(0, 0), algo="F16", tune_grid=2), 2,
         dict(family=1, entry=22, dtype=1, ig_mt_gt1=1, ig_roi=1, ig_roi_ragged=1, ig_sched=3)),
    _row("c037", "kitti_car/cascade-mscnn-7s-576-2x:roi_c1", dict(N=1, Cin=96, H=7, W=7, Cout=160, Kh=3, Kw=3, pad=(0, 0), algo="F16"), 2,
         dict(family=1, entry=22, dtype=1, ig_mt_gt1=1, ig_roi=1, ig_roi_ragged=1, ig_sched=4)),
    _row("c038", "kitti_ped_cyc/mscnn-7s-576-2x:roi_c1", dict(N=8, Cin=64, H=7, W=5, Cout=288, Kh=3, Kw=3, pad=(0, 0), algo="F16", tune_grid=2), 24,
         dict(family=1, entry=23, dtype=1, ig_mt_gt1=1, ig_roi=1, ig_sched=3)),
    _row("c039", "kitti_ped_cyc/mscnn-7s-576-2x:roi_c1", dict(N=8, Cin=96, H=7, W=5, Cout=160, Kh=3, Kw=3, pad=(0, 0), algo="F16"), 16,
         dict(family=1, entry=23, dtype=1, ig_mt_gt1=1, ig_roi=1, ig_sched=4)),
    _row("c040", "kitti_ped_cyc/mscnn-7s-576-2x:roi_c1", dict(N=1, Cin=96, H=7, W=5, Cout=160, Kh=3, Kw=3, pad=(0, 0), algo="F16"), 2,
         dict(family=1, entry=23, dtype=1, ig_mt_gt1=1, ig_roi=1, ig_roi_ragged=1, ig_sched=4)),
    _row("c041", "caltech/mscnn-7s-480:roi_c1", dict(N=8, Cin=64, H=8, W=4, Cout=160, Kh=3, Kw=3, pad=(1, 1), algo="F16", tune_grid=3), 16,
         dict(family=1, entry=24, dtype=1, ig_mt_gt1=1, ig_roi=1, ig_sched=3)),
    _row("c042", "caltech/mscnn-7s-480:roi_c1", dict(N=8, Cin=96, H=8, W=4, Cout=160, Kh=3, Kw=3, pad=(1, 1), algo="F16"), 12,
         dict(family=1, entry=24, dtype=1, ig_mt_gt1=1, ig_roi=1, ig_sched=4)),
    _row("c043", "caltech/mscnn-7s-480:roi_c1", dict(N=1, Cin=96, H=8, W=4, Cout=160, Kh=3, Kw=3, pad=(1, 1), algo="F16"), 2,
         dict(family=1, entry=24, dtype=1, ig_mt_gt1=1, ig_roi=1, ig_roi_ragged=1, ig_sched=4)),
    _row("c044", "kitti_car/mscnn-7s-576:roi_c1", dict(N=5, Cin=64, H=7, W=7, Cout=288, Kh=3, Kw=3, pad=(0, 0), algo="DIRECT", tune_grid=2), 15,
         dict(family=1, entry=31, ig_mt_gt1=1, ig_roi=1, ig_sched=3, publishes_amax=1)),
    _row("c045", "kitti_car/mscnn-7s-576:roi_c1", dict(N=5, Cin=64, H=7, W=7, Cout=160, Kh=3, Kw=3, pad=(0, 0), algo="AUTO"), 10,
         dict(family=1, entry=31, ig_mt_gt1=1, ig_roi=1, ig_sched=4, publishes_amax=1)),
    _row("c046", "kitti_car/mscnn-7s-576:roi_c1", dict(N=1, Cin=64, H=7, W=7, Cout=160, Kh=3, Kw=3, pad=(0, 0), algo="AUTO"), 2,
         dict(family=1, entry=31, ig_mt_gt1=1, ig_roi=1, ig_roi_ragged=1, ig_sched=4, publishes_amax=1)),
    _row("c047", "kitti_ped_cyc/mscnn-7s-576-2x:roi_c1", dict(N=8, Cin=64, H=7, W=5, Cout=288, Kh=3, Kw=3, pad=(0, 0), algo="DIRECT", tune_grid=2), 24,
         dict(family=1, entry=32, ig_mt_gt1=1, ig_roi=1, ig_sched=3, publishes_amax=1)),
    _row("c048", "kitti_ped_cyc/mscnn-7s-576-2x:roi_c1", dict(N=8, Cin=64, H=7, W=5, Cout=160, Kh=3, Kw=3, pad=(0, 0), algo="AUTO"), 16,
         dict(family=1, entry=32, ig_mt_gt1=1, ig_roi=1, ig_sched=4, publishes_amax=1)),
    _row("c049", "kitti_ped_cyc/mscnn-7s-576-2x:roi_c1", dict(N=1, Cin=64, H=7, W=5, Cout=160, Kh=3, Kw=3, pad=(0, 0), algo="AUTO"), 2,
         dict(family=1, entry=32, ig_mt_gt1=1, ig_roi=1, ig_roi_ragged=1, ig_sched=4, publishes_amax=1)),
    _row("c050", "caltech/mscnn-7s-480:roi_c1", dict(N=8, Cin=64, H=8, W=4, Cout=160, Kh=3, Kw=3, pad=(1, 1), algo="DIRECT", tune_grid=3), 16,
         dict(family=1, entry=33, ig_mt_gt1=1, ig_roi=1, ig_sched=3, publishes_amax=1)),
    _row("c051", "caltech/mscnn-7s-480:roi_c1", dict(N=8, Cin=64, H=8, W=4, Cout=160, Kh=3, Kw=3, pad=(1, 1), algo="AUTO"), 12,
         dict(family=1, entry=33, ig_mt_gt1=1, ig_roi=1, ig_sched=4, publishes_amax=1)),
    _row("c052", "caltech/mscnn-7s-480:roi_c1", dict(N=1, Cin=64, H=8, W=4, Cout=160, Kh=3, Kw=3, pad=(1, 1), algo="AUTO"), 2,
         dict(family=1, entry=33, ig_mt_gt1=1, ig_roi=1, ig_roi_ragged=1, ig_sched=4, publishes_amax=1)),
    _row("c053", "kitti_car/mscnn-7s-576:LFCN_4_5x5", dict(N=1, Cin=64, H=9, W=20, Cout=9, Kh=5, Kw=5, pad=(2, 2), algo="AUTO"), 2,
         dict(family=2, head_half=1, head_sched=1)),
    _row("c054", "kitti_car/mscnn-7s-576:LFCN_1_5x5", dict(N=2, Cin=96, H=18, W=65, Cout=9, Kh=5, Kw=5, pad=(2, 2), algo="AUTO"), 3,
         dict(family=2, head_half=1, head_sched=2)),
    _row("c055", "kitti_car/mscnn-7s-576:LFCN_2_7x7", dict(N=1, Cin=64, H=9, W=20, Cout=9, Kh=7, Kw=7, pad=(3, 3), algo="AUTO", tune_variant=500), 2,
         dict(family=2, entry=1, head_sched=2)),
    _row("c056", "kitti_car/mscnn-7s-576:LFCN_2_7x7", dict(N=1, Cin=96, H=18, W=65, Cout=9, Kh=7, Kw=7, pad=(3, 3), algo="AUTO"), 2,
         dict(family=2, entry=1, head_half=1, head_sched=2)),
    _row("c057", "caltech/mscnn-7s-480:LFCN_3_3x5", dict(N=1, Cin=64, H=9, W=20, Cout=6, Kh=5, Kw=3, pad=(2, 1), algo="AUTO"), 2,
         dict(family=2, entry=2, head_half=1, head_sched=1)),
    _row("c058", "caltech/mscnn-7s-480:LFCN_1_3x5", dict(N=2, Cin=96, H=18, W=65, Cout=6, Kh=5, Kw=3, pad=(2, 1), algo="AUTO"), 3,
         dict(family=2, entry=2, head_half=1, head_sched=2)),
    _row("c059", "caltech/mscnn-7s-480:LFCN_1_5x7", dict(N=1, Cin=64, H=9, W=20, Cout=6, Kh=7, Kw=5, pad=(3, 2), algo="AUTO", tune_variant=500), 2,
         dict(family=2, entry=3, head_sched=2)),
    _row("c060", "caltech/mscnn-7s-480:LFCN_3_5x7", dict(N=1, Cin=64, H=9, W=20, Cout=6, Kh=7, Kw=5, pad=(3, 2), algo="AUTO"), 2,
         dict(family=2, entry=3, head_half=1, head_sched=1)),
    _row("c061", "caltech/mscnn-7s-480:LFCN_1_5x7", dict(N=1, Cin=96, H=18, W=65, Cout=6, Kh=7, Kw=5, pad=(3, 2), algo="AUTO"), 2,
         dict(family=2, entry=3, head_half=1, head_sched=2)),
    _row("c062", "kitti_car/mscnn-7s-576:LFCN_1_7x7", dict(N=1, Cin=64, H=16, W=64, Cout=9, Kh=7, Kw=7, pad=(3, 3), algo="AUTO", tune_flags=1024), 2,
         dict(family=4, entry=30, ig_sched=4)),
    _row("c063", "caltech/mscnn-7s-480:LFCN_1_3x5", dict(N=1, Cin=64, H=9, W=20, Cout=6, Kh=5, Kw=3, pad=(2, 1), algo="WINO_F3_X3"), 2,
         dict(family=5, entry=-1, dtype=2)),
    _row("c064", "caltech/mscnn-7s-480:conv4_1", dict(N=2, Cin=96, H=33, W=16, Cout=288, Kh=3, Kw=3, pad=(1, 1), algo="AUTO", tune_variant=812), 3,
         dict(family=6, entry=1, wino_m=3, wino_gemm=2, wg_bm=256, wg_bn=128, wg_ck=32, wino_mt_gt1=1, wo_rem=1, publishes_amax=1)),
    _row("c065", "caltech/mscnn-7s-480:conv5_1", dict(N=2, Cin=96, H=36, W=16, Cout=288, Kh=3, Kw=3, pad=(1, 1), algo="AUTO", tune_variant=812), 3,
         dict(family=6, entry=1, wino_m=3, wino_gemm=2, wg_bm=256, wg_bn=128, wg_ck=32, wino_mt_gt1=1, wo_rem=1, can_pool=1, publishes_amax=1)),
    _row("c066", "widerface/cascade-mscnn-12s-align:conv5_1", dict(N=2, Cin=96, H=16, W=32, Cout=288, Kh=3, Kw=3, pad=(1, 1), algo="AUTO", tune_variant=812), 3,
         dict(family=6, entry=1, wino_m=3, wino_gemm=2, wg_bm=256, wg_bn=128, wg_ck=32, wino_mt_gt1=1, ho_rem=1, wo_rem=1, publishes_amax=1)),
    _row("c067", "widerface/cascade-mscnn-12s-align:conv4_1", dict(N=1, Cin=96, H=16, W=64, Cout=288, Kh=3, Kw=3, pad=(1, 1), algo="AUTO", tune_variant=812), 2,
         dict(family=6, entry=1, wino_m=3, wino_gemm=2, wg_bm=256, wg_bn=128, wg_ck=32, wino_mt_gt1=1, ho_rem=1, wo_rem=1, can_pool=1, publishes_amax=1)),
    _row("c068", "kitti_ped_cyc/mscnn-7s-576-2x:roi_c1", dict(N=65, Cin=64, H=7, W=5, Cout=288, Kh=3, Kw=3, pad=(0, 0), algo="WINO_F3", tune_variant=812), 66,
         dict(family=6, entry=1, wino_m=3, wino_gemm=2, wg_bm=256, wg_bn=128, wg_ck=32, wino_mt_gt1=1, wg_ragged=1, ho_rem=1, small_map=1, publishes_amax=1)),
    _row("c069", "caltech/mscnn-7s-480:roi_c1", dict(N=24, Cin=64, H=8, W=4, Cout=288, Kh=3, Kw=3, pad=(1, 1), algo="WINO_F3", tune_variant=812), 25,
         dict(family=6, entry=1, wino_m=3, wino_gemm=2, wg_bm=256, wg_bn=128, wg_ck=32, wino_mt_gt1=1, wg_ragged=3, ho_rem=1, wo_rem=1, small_map=1, publishes_amax=1)),
    _row("c070", "widerface/cascade-mscnn-12s-align:conv5_1", dict(N=2, Cin=96, H=64, W=49, Cout=288, Kh=3, Kw=3, pad=(1, 1), algo="AUTO", tune_variant=556), 3,
         dict(family=6, entry=1, wino_m=3, wino_gemm=2, wg_bm=256, wg_bn=128, wg_ck=32, wino_mt_gt1=1, wg_split=1, ho_rem=1, wo_rem=1, publishes_amax=1)),
    _row("c071", "widerface/cascade-mscnn-12s-align:conv4_2", dict(N=2, Cin=96, H=16, W=160, Cout=288, Kh=3, Kw=3, pad=(1, 1), algo="AUTO", tune_variant=556), 3,
         dict(family=6, entry=1, wino_m=3, wino_gemm=2, wg_bm=256, wg_bn=128, wg_ck=32, wino_mt_gt1=1, wg_split=1, ho_rem=1, wo_rem=1, can_pool=1, publishes_amax=1)),
    _row("c072", "kitti_ped_cyc/mscnn-7s-576-2x:roi_c1", dict(N=400, Cin=64, H=7, W=5, Cout=288, Kh=3, Kw=3, pad=(0, 0), algo="WINO_F3", tune_variant=556), 401,
         dict(family=6, entry=1, wino_m=3, wino_gemm=2, wg_bm=256, wg_bn=128, wg_ck=32, wino_mt_gt1=1, wg_split=1, wg_ragged=1, ho_rem=1, small_map=1, publishes_amax=1)),
    _row("c073", "caltech/mscnn-7s-480:roi_c1", dict(N=130, Cin=64, H=8, W=4, Cout=288, Kh=3, Kw=3, pad=(1, 1), algo="WINO_F3", tune_variant=556), 131,
         dict(family=6, entry=1, wino_m=3, wino_gemm=2, wg_bm=256, wg_bn=128, wg_ck=32, wino_mt_gt1=1, wg_split=1, wg_ragged=3, ho_rem=1, wo_rem=1, small_map=1, publishes_amax=1)),
    _row("c074", "caltech/mscnn-7s-480:conv3_1", dict(N=1, Cin=96, H=24, W=96, Cout=64, Kh=3, Kw=3, pad=(1, 1), algo="WINO_F4", tune_variant=301), 2,
         dict(family=6, entry=1, wino_m=4, wino_gemm=2, wg_bm=256, wg_bn=128, wg_ck=32, can_pool=1, can_pool_only=1, publishes_amax=1)),
    _row("c075", "kitti_car/mscnn-7s-384:conv3_2", dict(N=1, Cin=96, H=96, W=160, Cout=64, Kh=3, Kw=3, pad=(1, 1), algo="WINO_F4", tune_variant=557), 2,
         dict(family=6, entry=1, wino_m=4, wino_gemm=2, wg_bm=256, wg_bn=128, wg_ck=32, wg_split=1, can_pool=1, can_pool_only=1, publishes_amax=1)),
    _row("c076", "caltech/mscnn-7s-480:conv4_1", dict(N=1, Cin=96, H=24, W=96, Cout=288, Kh=3, Kw=3, pad=(1, 1), algo="WINO_F4", tune_variant=812), 2,
         dict(family=6, entry=1, wino_m=4, wino_gemm=2, wg_bm=256, wg_bn=128, wg_ck=32, wino_mt_gt1=1, can_pool=1, can_pool_only=1, publishes_amax=1)),
    _row("c077", "caltech/mscnn-7s-480:conv4_2", dict(N=2, Cin=96, H=36, W=96, Cout=288, Kh=3, Kw=3, pad=(1, 1), algo="WINO_F4", tune_variant=556), 3,
         dict(family=6, entry=1, wino_m=4, wino_gemm=2, wg_bm=256, wg_bn=128, wg_ck=32, wino_mt_gt1=1, wg_split=1, can_pool=1, can_pool_only=1, publishes_amax=1)),
    _row("c078", "citypersons/cascade-mscnn-8s-1344-2x:conv6_1", dict(N=2, Cin=96, H=17, W=160, Cout=288, Kh=3, Kw=3, pad=(1, 1), algo="WINO_F4", tune_variant=556), 3,
         dict(family=6, entry=1, wino_m=4, wino_gemm=2, wg_bm=256, wg_bn=128, wg_ck=32, wino_mt_gt1=1, wg_split=1, ho_rem=1, can_pool=1, can_pool_only=1, publishes_amax=1)),
    _row("c079", "caltech/mscnn-7s-480:conv2_1", dict(N=1, Cin=96, H=36, W=128, Cout=64, Kh=3, Kw=3, pad=(1, 1), algo="WINO_F4"), 2,
         dict(family=6, entry=2, wino_m=4, wino_gemm=2, wg_bm=128, wg_bn=256, wg_ck=32, can_pool=1, can_pool_only=1, publishes_amax=1)),
    _row("c080", "kitti_car/mscnn-7s-576:conv6_1", dict(N=1, Cin=96, H=36, W=48, Cout=160, Kh=3, Kw=3, pad=(1, 1), algo="AUTO", tune_variant=303), 2,
         dict(family=6, entry=3, wino_m=3, wino_gemm=2, wg_bm=128, wg_bn=128, wg_ck=32, wino_mt_gt1=1, can_pool=1, publishes_amax=1)),
    _row("c081", "kitti_car/mscnn-7s-384:conv5_1", dict(N=2, Cin=96, H=33, W=16, Cout=160, Kh=3, Kw=3, pad=(1, 1), algo="AUTO", tune_variant=303), 3,
         dict(family=6, entry=3, wino_m=3, wino_gemm=2, wg_bm=128, wg_bn=128, wg_ck=32, wino_mt_gt1=1, wo_rem=1, publishes_amax=1)),
    _row("c082", "kitti_car/mscnn-7s-384:conv6_1", dict(N=2, Cin=96, H=36, W=16, Cout=160, Kh=3, Kw=3, pad=(1, 1), algo="AUTO", tune_variant=303), 3,
         dict(family=6, entry=3, wino_m=3, wino_gemm=2, wg_bm=128, wg_bn=128, wg_ck=32, wino_mt_gt1=1, wo_rem=1, can_pool=1, publishes_amax=1)),
    _row("c083", "widerface/cascade-mscnn-12s-align:conv5_1", dict(N=2, Cin=96, H=16, W=32, Cout=160, Kh=3, Kw=3, pad=(1, 1), algo="AUTO", tune_variant=303), 3,
         dict(family=6, entry=3, wino_m=3, wino_gemm=2, wg_bm=128, wg_bn=128, wg_ck=32, wino_mt_gt1=1, ho_rem=1, wo_rem=1, publishes_amax=1)),
    _row("c084", "kitti_car/mscnn-7s-576:conv6_1", dict(N=1, Cin=96, H=36, W=48, Cout=160, Kh=3, Kw=3, pad=(1, 1), algo="AUTO", tune_variant=559), 2,
         dict(family=6, entry=3, wino_m=3, wino_gemm=2, wg_bm=128, wg_bn=128, wg_ck=32, wino_mt_gt1=1, wg_split=2, can_pool=1, publishes_amax=1)),
    _row("c085", "caltech/mscnn-7s-480:conv6_1", dict(N=2, Cin=96, H=33, W=16, Cout=160, Kh=3, Kw=3, pad=(1, 1), algo="AUTO", tune_variant=559), 3,
         dict(family=6, entry=3, wino_m=3, wino_gemm=2, wg_bm=128, wg_bn=128, wg_ck=32, wino_mt_gt1=1, wg_split=2, wo_rem=1, publishes_amax=1)),
    _row("c086", "kitti_car/mscnn-7s-384:conv6_1", dict(N=2, Cin=96, H=36, W=16, Cout=160, Kh=3, Kw=3, pad=(1, 1), algo="AUTO", tune_variant=559), 3,
         dict(family=6, entry=3, wino_m=3, wino_gemm=2, wg_bm=128, wg_bn=128, wg_ck=32, wino_mt_gt1=1, wg_split=2, wo_rem=1, can_pool=1, publishes_amax=1)),
    _row("c087", "widerface/cascade-mscnn-12s-align:conv5_1", dict(N=2, Cin=96, H=16, W=32, Cout=160, Kh=3, Kw=3, pad=(1, 1), algo="AUTO", tune_variant=559), 3,
         dict(family=6, entry=3, wino_m=3, wino_gemm=2, wg_bm=128, wg_bn=128, wg_ck=32, wino_mt_gt1=1, wg_split=2, ho_rem=1, wo_rem=1, publishes_amax=1)),
    _row("c088", "widerface/cascade-mscnn-12s-align:rpn_3_conv", dict(N=1, Cin=96, H=16, W=64, Cout=160, Kh=3, Kw=3, pad=(1, 1), algo="AUTO", tune_variant=559), 2,
         dict(family=6, entry=3, wino_m=3, wino_gemm=2, wg_bm=128, wg_bn=128, wg_ck=32, wino_mt_gt1=1, wg_split=2, ho_rem=1, wo_rem=1, can_pool=1, publishes_amax=1)),
    _row("c089", "caltech/mscnn-7s-480:roi_c1", dict(N=24, Cin=64, H=8, W=4, Cout=160, Kh=3, Kw=3, pad=(1, 1), algo="WINO_F3", tune_variant=559), 25,
         dict(family=6, entry=3, wino_m=3, wino_gemm=2, wg_bm=128, wg_bn=128, wg_ck=32, wino_mt_gt1=1, wg_split=2, wg_ragged=3, ho_rem=1, wo_rem=1, small_map=1, publishes_amax=1)),
    _row("c090", "kitti_car/mscnn-7s-576:conv5_1", dict(N=1, Cin=96, H=12, W=96, Cout=288, Kh=3, Kw=3, pad=(1, 1), algo="AUTO", tune_variant=304), 2,
         dict(family=6, entry=4, wino_m=3, wino_gemm=2, wg_bm=256, wg_bn=96, wg_ck=32, wino_mt_gt1=1, can_pool=1, publishes_amax=1)),
    _row("c091", "kitti_car/mscnn-7s-384:conv5_1", dict(N=2, Cin=96, H=9, W=49, Cout=288, Kh=3, Kw=3, pad=(1, 1), algo="AUTO", tune_variant=304), 3,
         dict(family=6, entry=4, wino_m=3, wino_gemm=2, wg_bm=256, wg_bn=96, wg_ck=32, wino_mt_gt1=1, wo_rem=1, publishes_amax=1)),
    _row("c092", "kitti_car/mscnn-7s-384:conv4_1", dict(N=2, Cin=96, H=36, W=16, Cout=288, Kh=3, Kw=3, pad=(1, 1), algo="AUTO", tune_variant=304), 3,
         dict(family=6, entry=4, wino_m=3, wino_gemm=2, wg_bm=256, wg_bn=96, wg_ck=32, wino_mt_gt1=1, wo_rem=1, can_pool=1, publishes_amax=1)),
    _row("c093", "caltech/mscnn-7s-480:conv6_1", dict(N=2, Cin=96, H=9, W=49, Cout=288, Kh=3, Kw=3, pad=(1, 1), algo="AUTO", tune_variant=560), 3,
         dict(family=6, entry=4, wino_m=3, wino_gemm=2, wg_bm=256, wg_bn=96, wg_ck=32, wino_mt_gt1=1, wg_split=2, wo_rem=1, publishes_amax=1)),
    _row("c094", "caltech/mscnn-7s-480:conv5_1", dict(N=2, Cin=96, H=36, W=16, Cout=288, Kh=3, Kw=3, pad=(1, 1), algo="AUTO", tune_variant=560), 3,
         dict(family=6, entry=4, wino_m=3, wino_gemm=2, wg_bm=256, wg_bn=96, wg_ck=32, wino_mt_gt1=1, wg_split=2, wo_rem=1, can_pool=1, publishes_amax=1)),
    _row("c095", "widerface/cascade-mscnn-12s-align:rpn_3_conv", dict(N=1, Cin=96, H=16, W=64, Cout=288, Kh=3, Kw=3, pad=(1, 1), algo="AUTO", tune_variant=560), 2,
         dict(family=6, entry=4, wino_m=3, wino_gemm=2, wg_bm=256, wg_bn=96, wg_ck=32, wino_mt_gt1=1, wg_split=2, ho_rem=1, wo_rem=1, can_pool=1, publishes_amax=1)),
    _row("c096", "kitti_ped_cyc/mscnn-7s-576-2x:roi_c1", dict(N=64, Cin=64, H=7, W=5, Cout=288, Kh=3, Kw=3, pad=(0, 0), algo="WINO_F3", tune_variant=560), 65,
         dict(family=6, entry=4, wino_m=3, wino_gemm=2, wg_bm=256, wg_bn=96, wg_ck=32, wino_mt_gt1=1, wg_split=2, wg_ragged=1, ho_rem=1, small_map=1, publishes_amax=1)),
    _row("c097", "caltech/mscnn-7s-480:roi_c1", dict(N=20, Cin=64, H=8, W=4, Cout=288, Kh=3, Kw=3, pad=(1, 1), algo="WINO_F3", tune_variant=560), 21,
         dict(family=6, entry=4, wino_m=3, wino_gemm=2, wg_bm=256, wg_bn=96, wg_ck=32, wino_mt_gt1=1, wg_split=2, wg_ragged=3, ho_rem=1, wo_rem=1, small_map=1, publishes_amax=1)),
    _row("c098", "caltech/mscnn-7s-480:conv3_1", dict(N=1, Cin=96, H=36, W=48, Cout=64, Kh=3, Kw=3, pad=(1, 1), algo="WINO_F4", tune_variant=304), 2,
         dict(family=6, entry=4, wino_m=4, wino_gemm=2, wg_bm=256, wg_bn=96, wg_ck=32, can_pool=1, can_pool_only=1, publishes_amax=1)),
    _row("c099", "citypersons/cascade-mscnn-8s-1344-2x:conv5_1", dict(N=1, Cin=96, H=36, W=48, Cout=288, Kh=3, Kw=3, pad=(1, 1), algo="AUTO", tune_variant=305), 2,
         dict(family=6, entry=5, wino_m=3, wino_gemm=2, wg_bm=256, wg_bn=160, wg_ck=32, wino_mt_gt1=1, can_pool=1, publishes_amax=1)),
    _row("c100", "caltech/mscnn-7s-480:roi_c1", dict(N=32, Cin=64, H=8, W=4, Cout=288, Kh=3, Kw=3, pad=(1, 1), algo="WINO_F3", tune_variant=305), 33,
         dict(family=6, entry=5, wino_m=3, wino_gemm=2, wg_bm=256, wg_bn=160, wg_ck=32, wino_mt_gt1=1, wg_ragged=3, ho_rem=1, wo_rem=1, small_map=1, publishes_amax=1)),
    _row("c101", "kitti_car/mscnn-7s-576:conv3_1", dict(N=1, Cin=96, H=24, W=128, Cout=64, Kh=3, Kw=3, pad=(1, 1), algo="WINO_F4", tune_variant=305), 2,
         dict(family=6, entry=5, wino_m=4, wino_gemm=2, wg_bm=256, wg_bn=160, wg_ck=32, can_pool=1, can_pool_only=1, publishes_amax=1)),
    _row("c102", "kitti_car/mscnn-7s-576:conv4_1", dict(N=1, Cin=96, H=24, W=128, Cout=288, Kh=3, Kw=3, pad=(1, 1), algo="WINO_F4", tune_variant=305), 2,
         dict(family=6, entry=5, wino_m=4, wino_gemm=2, wg_bm=256, wg_bn=160, wg_ck=32, wino_mt_gt1=1, can_pool=1, can_pool_only=1, publishes_amax=1)),
    _row("c103", "kitti_car/mscnn-7s-576:conv4_2", dict(N=1, Cin=96, H=64, W=128, Cout=288, Kh=3, Kw=3, pad=(1, 1), algo="WINO_F4", tune_variant=561), 2,
         dict(family=6, entry=5, wino_m=4, wino_gemm=2, wg_bm=256, wg_bn=160, wg_ck=32, wino_mt_gt1=1, wg_split=1, can_pool=1, can_pool_only=1, publishes_amax=1)),
    _row("c104", "kitti_car/mscnn-7s-576:conv2_1", dict(N=1, Cin=96, H=12, W=32, Cout=64, Kh=3, Kw=3, pad=(1, 1), algo="WINO_F4", tune_grid=1, tune_flags=128), 2,
         dict(family=6, entry=9, ig_sched=1, wino_m=4, wino_gemm=1, can_pool=1, can_pool_only=1, publishes_amax=1)),
    _row("c105", "citypersons/cascade-mscnn-8s-1344-2x:conv3_1", dict(N=1, Cin=96, H=12, W=48, Cout=288, Kh=3, Kw=3, pad=(1, 1), algo="AUTO", tune_grid=1, tune_flags=128), 2,
         dict(family=6, entry=9, ig_mt_gt1=1, ig_sched=1, wino_m=3, wino_gemm=1, can_pool=1, publishes_amax=1)),
    _row("c106", "citypersons/cascade-mscnn-8s-1344-2x:conv3_1", dict(N=1, Cin=96, H=12, W=32, Cout=288, Kh=3, Kw=3, pad=(1, 1), algo="WINO_F4", tune_grid=1, tune_flags=128), 2,
         dict(family=6, entry=9, ig_mt_gt1=1, ig_sched=1, wino_m=4, wino_gemm=1, can_pool=1, can_pool_only=1, publishes_amax=1)),
    _row("c107", "citypersons/cascade-mscnn-8s-1344-2x:conv3_1", dict(N=1, Cin=96, H=36, W=48, Cout=160, Kh=3, Kw=3, pad=(1, 1), algo="WINO_F3_X3", tune_flags=4), 2,
         dict(family=7, entry=128, dtype=2, wino_m=3, wino_gemm=3, wino_mt_gt1=1, can_pool=1, publishes_amax=1)),
    _row("c108", "caltech/mscnn-7s-480:conv4_1", dict(N=2, Cin=96, H=33, W=16, Cout=160, Kh=3, Kw=3, pad=(1, 1), algo="WINO_F3_X3", tune_flags=4), 3,
         dict(family=7, entry=128, dtype=2, wino_m=3, wino_gemm=3, wino_mt_gt1=1, wo_rem=1, publishes_amax=1)),
    _row("c109", "caltech/mscnn-7s-480:conv3_1", dict(N=2, Cin=96, H=36, W=16, Cout=160, Kh=3, Kw=3, pad=(1, 1), algo="WINO_F3_X3", tune_flags=4), 3,
         dict(family=7, entry=128, dtype=2, wino_m=3, wino_gemm=3, wino_mt_gt1=1, wo_rem=1, can_pool=1, publishes_amax=1)),
    _row("c110", "kitti_ped_cyc/mscnn-7s-576-2x:roi_c1", dict(N=65, Cin=64, H=7, W=5, Cout=160, Kh=3, Kw=3, pad=(0, 0), algo="WINO_F3_X3", tune_flags=4), 66,
         dict(family=7, entry=128, dtype=2, wino_m=3, wino_gemm=3, wino_mt_gt1=1, ho_rem=1, small_map=1, publishes_amax=1)),
    _row("c111", "widerface/cascade-mscnn-12s-align:conv3_1", dict(N=2, Cin=96, H=16, W=32, Cout=160, Kh=3, Kw=3, pad=(1, 1), algo="WINO_F3_X3", tune_flags=4), 3,
         dict(family=7, entry=128, dtype=2, wino_m=3, wino_gemm=3, wino_mt_gt1=1, ho_rem=1, wo_rem=1, publishes_amax=1)),
    _row("c112", "widerface/cascade-mscnn-12s-align:conv4_1", dict(N=1, Cin=96, H=16, W=64, Cout=160, Kh=3, Kw=3, pad=(1, 1), algo="WINO_F3_X3", tune_flags=4), 2,
         dict(family=7, entry=128, dtype=2, wino_m=3, wino_gemm=3, wino_mt_gt1=1, ho_rem=1, wo_rem=1, can_pool=1, publishes_amax=1)),
    _row("c113", "caltech/mscnn-7s-480:roi_c1", dict(N=24, Cin=64, H=8, W=4, Cout=160, Kh=3, Kw=3, pad=(1, 1), algo="WINO_F3_X3", tune_flags=4), 25,
         dict(family=7, entry=128, dtype=2, wino_m=3, wino_gemm=3, wino_mt_gt1=1, ho_rem=1, wo_rem=1, small_map=1, publishes_amax=1)),
    _row("c114", "caltech/mscnn-7s-480:conv1_1", dict(N=1, Cin=3, H=64, W=64, Cout=16, Kh=3, Kw=3, pad=(1, 1), algo="AUTO"), 2,
         dict(family=8, entry=-1, publishes_amax=1, c3=1)),
    _row("c115", "caltech/mscnn-7s-480:conv1_2", dict(N=1, Cin=64, H=64, W=128, Cout=64, Kh=3, Kw=3, pad=(1, 1), algo="AUTO", tune_variant=403), 2,
         dict(family=9, entry=-1, can_pool=1, can_pool_only=1, wf_use=1)),
    _row("c116", "caltech/mscnn-7s-480:conv1_2", dict(N=1, Cin=64, H=64, W=128, Cout=64, Kh=3, Kw=3, pad=(1, 1), algo="AUTO", tune_variant=402), 2,
         dict(family=10, entry=2, can_pool=1, can_pool_only=1, wc_use=1)),
]

# class (tuple, as class_of_row gives it) -> why no desc within the caps plans to it.  Empty: every class of the census has a row.
UNREACHED = {}


def listing():
    """The census as a table for readers (tests/CONV_CLASSES.md holds it; the CPU test keeps the file equal to this)."""
    cen = census()
    by_class = {}
    for r in CASES:
        by_class.setdefault(class_of_row(r), []).append(r)
    out = ["# Convolution plan classes of the deploy nets", "",
           "Generated by `python tests/conv_classes.py > tests/CONV_CLASSES.md`; `tests/test_conv_class_census_cpu.py` fails when this file is stale.",
           "", f"Every model of `mscnn_amd.zoo.MODELS` at its shipped size, batch {', '.join(map(str, BATCHES))}, algos {', '.join(NET_ALGOS)};",
           f"layers fed by ROIs at R = {', '.join(map(str, ROI_COUNTS))}.  {len(cen)} classes, {len(CASES)} rows, {len(UNREACHED)} unreached.",
           "A class lists its non-zero fields; `layers` counts distinct (model, layer) pairs, `plans` every (model, layer, algo, batch or R).", "",
           "| row | class | layers | plans | algos | stands for | desc of the row |", "|---|---|---|---|---|---|---|"]
    for c in sorted(cen):
        rows = by_class.get(c, [])
        ex = cen[c]
        layers = len({(m, l) for m, l, *_ in ex})
        algos = "/".join(a for a in NET_ALGOS if any(e[2] == a for e in ex))
        rid = ", ".join(r["id"] for r in rows) or ("UNREACHED: " + UNREACHED[c] if c in UNREACHED else "none")
        desc = "; ".join(", ".join(f"{k}={v}" for k, v in r["desc"].items()) + f", N2={r['N2']}" for r in rows)
        out.append(f"| {rid} | {brief(c)} | {layers} | {len(ex)} | {algos} | {rows[0]['layer'] if rows else ex[0][0] + ':' + ex[0][1]} | {desc} |")
    return "\n".join(out) + "\n"


if __name__ == "__main__":
    sys.stdout.write(listing())
