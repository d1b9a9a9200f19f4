"""Shapes, integer operands and the list of weight writers of tests/test_weight_state.py (CPU) and tests/test_weight_state_gpu.py.

What is under test is the state BETWEEN the modules and the convolution kernels: native._PACK_CACHE (GEMM-ready and Winograd-transformed
copies of every conv weight), native.conv2d_pack_all (all copies of a FlatParams bucket in one launch behind FlatAdam.step), the
re-homing of parameters into a bucket, and the folded weights of a frozen conv / BN pair.  Every case warms that state, writes the
weights, and convolves again: the result must be the convolution with the weights the module holds NOW.

Integer weights live in [0, 3] and a writer that can write integers writes 3 - w: every element changes (3 - w = w has no integer
solution), so a stale copy is wrong in every output element whose receptive field holds a non-zero input.  With |x|, |dy| <= 4 and
at most 32 * 9 terms the magnitude sums, those of the Winograd transform chain included, stay below 2^14 (the tests assert
4 max S < 2^24): every path is exact."""
import torch

import conv_refs as R

# name -> (Cin, Cout, k, pad)
LAYERS = {
    "c32": (32, 32, 3, 1),       # min(C, M) = WINO_MIN_C: Winograd on even maps, implicit GEMM on odd ones
    "p1x1": (32, 16, 1, 0),      # 1x1: never Winograd
    "c16": (16, 32, 3, 1),       # 3x3 below WINO_MIN_C: never Winograd
}
# the four consumers of a derived copy, two per call (forward + data gradient): (layer, H, W, route); route "wino" reads the layouts
# 2 and 3 of the pack cache, "gemm" the layouts 0 (False) and 1 (True)
CALLS = [("c32", 8, 8, "wino"), ("c32", 7, 8, "gemm"), ("p1x1", 8, 8, "gemm"), ("c16", 8, 8, "gemm")]
CALL_IDS = ["%s-%dx%d-%s" % c for c in CALLS]
LAYOUTS = {"wino": (2, 3), "gemm": (False, True)}

# writers of a weight inside a FlatParams bucket / of a Parameter outside every bucket
# (the sixth writer, FlatParams(module, keep_grads=True) behind the first backward, re-homes the weight instead of changing its values:
#  test_weight_state_gpu.test_flattening_after_the_first_backward_rehomes_the_weight is its test)
BUCKET_WRITERS = ["adam_step", "param_copy", "load_state_dict", "bucket_copy", "checkpoint_restore"]
PLAIN_WRITERS = ["param_copy", "load_state_dict", "raw_write_weight_epoch"]

W_MAX = 3


def int_weight(name, seed=0):
    Cin, Cout, k, _ = LAYERS[name]
    return R.ints((Cout, Cin, k, k), 0, W_MAX, 1000 + 17 * seed + sorted(LAYERS).index(name))


def flipped(w):
    """integers again, different from w in every element"""
    return W_MAX - w


def int_operands(call, seed=0):
    """x [1, Cin, H, W] and dy [1, Cout, OH, OW] (stride 1, 'same' padding: OH = H) of a CALLS entry"""
    name, H, W, _ = call
    Cin, Cout, k, _ = LAYERS[name]
    return R.ints((1, Cin, H, W), -R.INT_X, R.INT_X, 2000 + seed), R.ints((1, Cout, H, W), -R.INT_X, R.INT_X, 3000 + seed)


def refs(call, w, x, dy):
    """-> (forward, data gradient): f(dtype) -> (value, S) of tests/conv_refs.py for the weights `w` (a CPU tensor read back from the
    module after the write), the Winograd restatement where the call runs the Winograd kernels"""
    name, H, W, route = call
    pad = LAYERS[name][3]
    if route == "wino":
        return (lambda dt: R.wino_fwd(x, w, None, dtype=dt)), (lambda dt: R.wino_dgrad(dy, w, dtype=dt))
    return (lambda dt: R.conv_fwd(x, w, None, 1, pad, dtype=dt)), (lambda dt: R.conv_dgrad(dy, w, tuple(x.shape), 1, pad, dtype=dt))


def chain_terms(call):
    """K of rule A (tests/test_conv_edges_gpu.py: direct_K / wino_K) for the forward and the data gradient of a CALLS entry"""
    name, H, W, route = call
    Cin, Cout, k, _ = LAYERS[name]
    return (9 * Cin + 8, 9 * Cout + 8) if route == "wino" else (Cin * k * k + 1, Cout * k * k)


# ---- the frozen conv / BN pair of folded_conv_bn: conv(8 -> 8, 3x3, no bias) + eval-mode BatchNorm, map 6 x 6
FOLD_C, FOLD_HW = 8, 6
# eps = 0 and variances that are powers of 4: sqrt(var) is a power of two, so k = gamma / sqrt(var) is a dyadic rational with at most
# 3 significant bits, w' = w k and b' = beta - mean k are exact products and sums of such numbers, and with integer x every partial
# sum of the folded convolution is a multiple of 2^-6 below 2^13: exact in fp32 in any order, as is BN(conv(x)) in fp64
FOLD_VAR = [(0.25, 1.0, 4.0, 16.0, 1.0, 0.25, 4.0, 1.0), (4.0, 0.25, 1.0, 1.0, 16.0, 4.0, 0.25, 16.0)]
FOLD_GAMMA = [(1.0, 0.5, -1.0, 2.0, 1.5, -0.5, 1.0, 0.75), (-1.0, 1.5, 0.5, 1.0, -2.0, 0.75, 2.0, 0.5)]
FOLD_BETA = [(0.0, 0.5, -1.0, 2.0, -0.25, 1.0, 0.0, 3.0), (1.0, -0.5, 0.25, 0.0, 2.0, -3.0, 0.5, 1.0)]
FOLD_MEAN = [(1.0, -2.0, 0.5, 0.0, 3.0, -1.0, 2.0, 0.25), (-1.0, 0.5, 2.0, 1.0, 0.0, 3.0, -0.5, -2.0)]


def fold_state(which, weight_seed=0):
    """state_dict of nn.Sequential(conv, bn) for the value set `which` (0 / 1: the two differ in every element)"""
    w = R.ints((FOLD_C, FOLD_C, 3, 3), 0, W_MAX, 4000 + weight_seed)
    return {"0.weight": flipped(w) if which else w, "1.weight": torch.tensor(FOLD_GAMMA[which]), "1.bias": torch.tensor(FOLD_BETA[which]),
            "1.running_mean": torch.tensor(FOLD_MEAN[which]), "1.running_var": torch.tensor(FOLD_VAR[which])}


def fold_ref(state, x, dtype=torch.float64):
    """relu(BN_eval(conv(x))) in `dtype`, eps = 0, from a fold_state-shaped dict of CPU tensors"""
    s = {k: v.to(dtype) for k, v in state.items() if v.is_floating_point()}
    y = torch.nn.functional.conv2d(x.to(dtype), s["0.weight"], None, padding=1)
    c = lambda t: t.view(1, -1, 1, 1)
    return torch.relu((y - c(s["1.running_mean"])) / torch.sqrt(c(s["1.running_var"])) * c(s["1.weight"]) + c(s["1.bias"]))


def fold_ref_params(state, dtype=torch.float64):
    """(w', b') of the fold in `dtype`"""
    s = {k: v.to(dtype) for k, v in state.items() if v.is_floating_point()}
    k = s["1.weight"] / torch.sqrt(s["1.running_var"])
    return s["0.weight"] * k.view(-1, 1, 1, 1), s["1.bias"] - s["1.running_mean"] * k
