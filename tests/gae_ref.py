"""numpy restatement of gae.hip's welford_combine_kernel: Chan's combine in the operation order of the reference's
welford_var.h (csrc/reduce.h chan_ref_order) folded in the runs-then-tree order (csrc/reduce.h fold_runs_tree).
Every operation is one IEEE double operation, written in the order the device evaluates it; shares nothing with csrc.
"""
import numpy as np

F64 = np.float64
LANES = 256


def chan_ref_order(a, b):
    """a ⊕ b on (n, mean, M2): mean + (δ·nb)/nn, M2 + (M2b + (((δ·δ)·n)·nb)/nn); an empty side leaves the other."""
    n, mean, m2 = (F64(v) for v in a)
    nb, mb, m2b = (F64(v) for v in b)
    if nb <= 0.0:
        return n, mean, m2
    if n <= 0.0:
        return nb, mb, m2b
    nn = n + nb
    d = mb - mean
    return nn, mean + d * nb / nn, m2 + (m2b + d * d * n * nb / nn)


def fold_runs_tree(parts, combine, lanes=LANES):
    """Lane t folds parts [t·per, (t+1)·per), per = ⌈count/lanes⌉, in index order from the zero triple; then the
    pairwise tree, stride 1, 2, 4, …: lane t, a multiple of 2·stride, takes lane t + stride."""
    count = len(parts)
    per = (count + lanes - 1) // lanes
    zero = (F64(0.0), F64(0.0), F64(0.0))
    s = []
    for t in range(lanes):
        a = zero
        for i in range(t * per, min(count, (t + 1) * per)):
            a = combine(a, parts[i])
        s.append(a)
    stride = 1
    while stride < lanes:
        for t in range(0, lanes, 2 * stride):
            s[t] = combine(s[t], s[t + stride])
        stride *= 2
    return np.array(s[0], F64)
