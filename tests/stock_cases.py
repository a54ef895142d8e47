"""The parameter space of the stock layers (ReLU, MAX/AVE pooling, Softmax, transposed convolution, Eltwise, Concat), stated once:
tests/test_oracle_vs_ref.py sweeps it oracle against reference, tests/golden/make_golden_c.py records a subset of it from the
reference, tests/test_golden.py replays that subset and tests/test_gpu_stock_layers.py runs it HIP against oracle.  Inputs only: every
function here is deterministic in its arguments, nothing here computes an expected value."""
import itertools

import numpy as np

# ------------------------------------------------------------------------------------------------ pooling
POOL_SIZES = [(H, W) for H in (3, 5, 6, 7, 9) for W in (4, 5, 7, 8)]        # the CPU sweep
POOL_SIZES_GPU = [(3, 4), (7, 8)]
POOL_PLANES = (1, 2)                                                          # N, C of every swept map


def pool_params():
    """(kernel, pad, stride) with kernel, stride in {1,2,3} and 0 <= pad < kernel per dimension: 18 x 18 = 324."""
    one = [(k, p, s) for k in (1, 2, 3) for p in range(k) for s in (1, 2, 3)]
    return [((a[0], b[0]), (a[1], b[1]), (a[2], b[2])) for a, b in itertools.product(one, one)]


def pool_input(H, W):
    return np.random.default_rng(1000 * H + W).standard_normal(POOL_PLANES + (H, W)).astype(np.float32)


def pool_dims_per_dimension(H, W, kernel, pad, stride):
    """The rule this project had before the pin: each dimension clipped on its OWN pad only.  Kept to SELECT the cases where
    the reference's both-pads rule matters, never as an expectation."""
    out = []
    for i, k, p, s in zip((H, W), kernel, pad, stride):
        o = -((i + 2 * p - k) // -s) + 1
        if p and (o - 1) * s >= i + p:
            o -= 1
        out.append(o)
    return tuple(out)


# ------------------------------------------------------------------------------------------------ ReLU
RELU_SLOPES = (0.0, 0.1, -0.5)
RELU_SPECIALS = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1e-40, -1e-40, 3.0, -3.0], np.float32)
RELU_SPECIALS_DEVICE = RELU_SPECIALS[:5]         # +-0, +-inf, NaN (what the device does with denormals is not measured)


def bits(a):
    """Bit patterns with every NaN mapped to one pattern.  IEEE 754 leaves the sign and payload of a NaN that an invalid
    operation produces (0 * inf) to the implementation: x86 SSE gives the negative default NaN, gfx950 the positive one.
    Everything else -- signed zeros, infinities, denormals, normals -- is compared bit for bit."""
    a = np.ascontiguousarray(a, np.float32)
    u = a.view(np.uint32).copy()
    u[np.isnan(a)] = 0x7FC00000
    return u


# ------------------------------------------------------------------------------------------------ Softmax
SOFTMAX_SHAPES = [(3, 5, 4, 6), (2, 3, 7), (2, 300, 3), (1, 5, 1, 1)]
SOFTMAX_SCALES = (1.0, 30.0, 100.0)
SOFTMAX_SPECIALS = ("inf", "nan", "all_ninf", "pm1000")


def softmax_inputs():
    """[(tag, x)]: every shape at every scale, and per shape four inputs whose row at position (0, .., 0) holds a special."""
    out = []
    for si, shape in enumerate(SOFTMAX_SHAPES):
        rng = np.random.default_rng(4000 + si)
        for scale in SOFTMAX_SCALES:
            out.append((f"s{si}_x{int(scale)}", (rng.standard_normal(shape) * scale).astype(np.float32)))
        for kind in SOFTMAX_SPECIALS:
            x = rng.standard_normal(shape).astype(np.float32)
            row = x[(0, slice(None)) + (0,) * (len(shape) - 2)]                   # the C values of the first (outer, inner) position
            if kind == "inf":
                row[1] = np.inf
            elif kind == "nan":
                row[shape[1] // 2] = np.nan
            elif kind == "all_ninf":
                row[:] = -np.inf
            else:
                row[0::2] = 1000.0; row[1::2] = -1000.0
            out.append((f"s{si}_{kind}", x))
    return out


# ------------------------------------------------------------------------------------------------ transposed convolution
DECONV_CIN, DECONV_HW = 4, (5, 6)
DECONV_FAMILIES = {"g1": (1, 6), "g2": (2, 6), "gcin": (4, 8), "dw": (4, 4)}     # name -> (group, Cout); dw = the depthwise kernels


def deconv_cases():
    """[(family, kernel, stride, pad, bias)]: kernels (3,5) (5,3) (1,1), strides (1,3) (3,2), pad 0 and kernel // 2."""
    out = []
    for fam in DECONV_FAMILIES:
        for k in ((3, 5), (5, 3), (1, 1)):
            for s in ((1, 3), (3, 2)):
                for p in sorted({(0, 0), (k[0] // 2, k[1] // 2)}):
                    for bias in (False, True):
                        out.append((fam, k, s, p, bias))
    return out


def deconv_inputs(case, index):
    fam, k, s, p, bias = case
    group, cout = DECONV_FAMILIES[fam]
    rng = np.random.default_rng(5000 + index)
    x = rng.standard_normal((2, DECONV_CIN) + DECONV_HW).astype(np.float32)
    w = (rng.standard_normal((DECONV_CIN, cout // group) + k) * 0.5).astype(np.float32)
    b = rng.standard_normal(cout).astype(np.float32) if bias else None
    return x, w, b, group


# ------------------------------------------------------------------------------------------------ Eltwise
ELTWISE_BOTTOMS = (2, 3, 5, 8)
ELTWISE_COEFFS = {2: [-1.5, 0.0], 3: [0.25, 0.0, -2.0], 5: [1.0, -1.0, 0.0, 0.5, 3.0], 8: [0.5, -0.25, 0.0, 2.0, -1.0, 1.0, 0.125, -3.0]}


def eltwise_inputs(nb, shape=(7, 5)):
    """nb bottoms; every third element repeats bottom 0's value in bottom 1 and the last bottom (MAX ties)."""
    rng = np.random.default_rng(6000 + nb)
    xs = [rng.standard_normal(shape).astype(np.float32) for _ in range(nb)]
    xs[1].reshape(-1)[::3] = xs[0].reshape(-1)[::3]
    xs[-1].reshape(-1)[::3] = xs[0].reshape(-1)[::3]
    return xs


# ------------------------------------------------------------------------------------------------ Concat
def concat_cases():
    """[(axis, [three arrays])]: per axis 0, 1, 2 one case with a trailing block (inner > 1) and one whose axis is the last (inner 1)."""
    rng = np.random.default_rng(7000)
    out = []
    for axis in (0, 1, 2):
        for base in ((2, 3, 4, 5), (2, 3, 4, 5)[:axis + 1]):
            xs = []
            for extent in (2, 1, 3):
                shape = list(base); shape[axis] = extent
                xs.append(rng.standard_normal(shape).astype(np.float32))
            out.append((axis, xs))
    return out
