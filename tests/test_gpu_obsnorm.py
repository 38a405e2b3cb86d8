"""Running observation normalisation in the device PPO update (ppo_set_obs_norm, csrc/obsnorm.hip).

The oracle has no such option: the reference is tests/obsnorm_ref.py (pinned on the CPU in test_obsnorm_cpu.py,
which also holds the statistics cases and their bounds).  The update is checked against itself: an update with
the feature on over a raw buffer must equal an update with it off over the buffer normalised on the host by the
bit-comparable fp32 model — the same kernels run on the same bits.
"""
import ctypes as C

import numpy as np
import pytest

import ppo_ffi
import test_gpu_rollout
from helpers import F32, assert_gemm_close, dev, empty, nn_grads_packed, nn_input_rows, nn_params_packed
from obsnorm_ref import affine, chan, normalize_f32, stats64
from test_gpu_update import make_ppo
from test_obsnorm_cpu import STATS_SHAPES, check_triple, chunked64, stats_case

pytestmark = pytest.mark.gpu

SEED = 77
NSTAT = 22


def stats(lib, ppo, n=NSTAT):
    st = (C.c_double * n)()
    lib.ppo_read_stats(ppo, st, n)
    return list(st)


def set_state(lib, ppo, triple):
    t = np.ascontiguousarray(triple, np.float64)
    return lib.ppo_obs_norm_set_state(ppo, t.ctypes.data_as(C.POINTER(C.c_double)), t.size)


def get_state(lib, ppo, S):
    out = (C.c_double * (1 + 2 * S))()
    assert lib.ppo_obs_norm_get_state(ppo, out, 1 + 2 * S) == 1 + 2 * S
    return np.array(out[:])


def dev_affine(lib, ppo, S):
    m, r = np.empty(S, F32), np.empty(S, F32)
    assert lib.ppo_obs_norm_affine(ppo, m.ctypes.data, r.ctypes.data, S) == 0
    return m, r


def known_triple(S, mean, std, n=5000.0):
    mean, std = np.broadcast_to(np.asarray(mean, np.float64), S), np.broadcast_to(np.asarray(std, np.float64), S)
    return np.concatenate([[n], mean, n * std * std])


def no_error(lib):
    assert lib.ppo_last_error() in (b"", None), lib.ppo_last_error()


# ----------------------------------------------------------------------------- 1. the statistics kernel alone
def dev_stats(lib, dx, n, S):
    out = (C.c_double * (1 + 2 * S))()
    assert lib.ppo_obs_stats_device(dx.ptr, n, S, out) == 0
    return np.array(out[:])


@pytest.mark.parametrize("n,S", STATS_SHAPES)
def test_stats_kernel(lib, n, S):
    x, kinds, ref = stats_case(n, S)
    # the same algorithm class on the CPU stays inside the bounds
    check_triple(chunked64(x, 64), ref, kinds, f"float64 chunks, {n} x {S}")
    dx = dev(lib, x)
    a = dev_stats(lib, dx, n, S)
    b = dev_stats(lib, dx, n, S)
    dx.free()
    worst = check_triple(a, ref, kinds, f"ppo_obs_stats_device {n} x {S}")
    print(f"{n} x {S}: worst (mean err / std, M2 rel err) {worst}")
    np.testing.assert_array_equal(a.view(np.uint64), b.view(np.uint64))
    no_error(lib)


def test_stats_bad_arguments(lib):
    out = (C.c_double * 7)()
    d = empty(lib, 12)
    assert lib.ppo_obs_stats_device(d.ptr, 4, 0, out) == -1
    assert lib.ppo_obs_stats_device(None, 4, 3, out) == -1
    assert lib.ppo_obs_stats_device(d.ptr, -1, 3, out) == -1
    assert lib.ppo_obs_stats_device(d.ptr, 0, 3, out) == 0 and list(out) == [0.0] * 7
    d.free()


# ----------------------------------------------------------------------------- 2. affine pair and normalisation
def norm_dev(lib, ppo, x, in_place):
    n, S = x.shape
    dx = dev(lib, x)
    dy = dx if in_place else empty(lib, n * S)
    assert lib.ppo_obs_normalize_device(ppo, dx.ptr, dy.ptr, n) == 0
    y = dy.to_numpy(F32, n * S).reshape(n, S)
    if not in_place:
        np.testing.assert_array_equal(dx.to_numpy(F32, n * S).reshape(n, S).view(np.uint32), x.view(np.uint32))
        dy.free()
    dx.free()
    return y


@pytest.mark.parametrize("n,S", [(1, 3), (7, 5), (4099, 376)])
def test_affine_and_normalize(lib, oracle, n, S):
    rng = np.random.default_rng(50 + S)
    ppo = make_ppo(lib, oracle, [S, 16, 2], 8)
    mean = rng.normal(size=S) * 10.0 ** rng.uniform(-1, 2, S)
    std = 10.0 ** rng.uniform(-2, 2, S)
    tri = known_triple(S, mean, std, n=12345.0)
    x = (mean + std * rng.normal(size=(n, S))).astype(F32)
    if n > 1:
        x[n // 2, S // 2] = np.nan
    assert lib.ppo_set_obs_norm(ppo, 10.0) == 0
    # un-warmed: the identity bit for bit, even with clip 0.5
    assert lib.ppo_set_obs_norm(ppo, 0.5) == 0
    y = norm_dev(lib, ppo, x, False)
    np.testing.assert_array_equal(y.view(np.uint32), x.view(np.uint32))
    assert stats(lib, ppo)[19:] == [0, 0, 0]
    # the pair of a known triple
    assert set_state(lib, ppo, tri) == 0
    np.testing.assert_array_equal(get_state(lib, ppo, S), tri)
    m, r = dev_affine(lib, ppo, S)
    np.testing.assert_array_equal(m, tri[1:1 + S].astype(F32))
    r_ref = (1 / np.sqrt(tri[1 + S:] / tri[0] + 1e-8)).astype(F32)
    assert (np.abs(r.astype(np.float64) - r_ref) <= np.spacing(r_ref)).all()
    np.testing.assert_array_equal(affine(tri)[0], m)
    for clip in (10.0, 0.5, float("inf")):
        assert lib.ppo_set_obs_norm(ppo, clip) == 0 and lib.ppo_get_obs_norm(ppo) == F32(clip)
        y_ref, cl = normalize_f32(x, m, r, clip)
        if clip == 0.5 and n > 1:
            assert 0.1 < cl.mean() < 0.9, cl.mean()
        for in_place in (False, True):
            y = norm_dev(lib, ppo, x, in_place)
            np.testing.assert_array_equal(y.view(np.uint32), y_ref.view(np.uint32))
            # the call counts nothing: out[20] / out[21] describe updates (test_clamp_boundary_… counts through one)
            assert stats(lib, ppo)[19:] == [tri[0], 0, 0]
        if n > 1:
            assert np.isnan(y[n // 2, S // 2]) and not cl[n // 2, S // 2]
        if clip == float("inf"):
            assert not cl.any()
    no_error(lib)
    lib.free_ppo(ppo)


def test_clamp_boundary_and_bad_arguments(lib, oracle):
    S = 5
    ppo = make_ppo(lib, oracle, [S, 16, 2], 8)
    assert lib.ppo_get_obs_norm(ppo) == 0.0
    d = empty(lib, 8 * S)
    assert lib.ppo_obs_normalize_device(ppo, d.ptr, d.ptr, 8) == -1          # off
    assert lib.ppo_obs_norm_fold_buffer(ppo) == -1
    assert stats(lib, ppo)[19:] == [0, 0, 0]
    assert lib.ppo_set_obs_norm(ppo, 0.5) == 0
    # m = 0, r = 1 exactly: elements exactly at ±c pass through and are not counted
    tri = known_triple(S, 0.0, 1.0, n=4.0)
    tri[1 + S:] = 4.0 * (1.0 - 1e-8)
    assert set_state(lib, ppo, tri) == 0
    m, r = dev_affine(lib, ppo, S)
    assert (m == 0).all() and (r == 1).all()
    x = np.array([[0.5, -0.5, 0.25, 0.50000006, -0.75]] * 8, F32)
    y = norm_dev(lib, ppo, x, True)
    y_ref, cl = normalize_f32(x, m, r, 0.5)
    np.testing.assert_array_equal(y, y_ref)
    assert cl[0].tolist() == [False, False, False, True, True]
    # counted where the counters are defined: by an update's state normalisation over these rows (GAE only)
    lib.ppo_fill_synthetic(ppo, 2, 4, 3, 0.0)
    lib.ppo_synchronize()
    ppo_ffi.h2d(lib, ppo.contents.buffer.contents.d_state_p, x)
    assert lib.ppo_obs_norm_freeze(ppo, 1) == 0
    lib.ppo_set_step_limit(ppo, 0, 0)
    lib.ppo_update(ppo, 0.99, 8, 1, 1, 1, SEED)
    lib.ppo_synchronize()
    assert stats(lib, ppo)[19:] == [4, cl.sum(), 8 * S] and cl.sum() == 16
    lib.ppo_set_step_limit(ppo, -1, -1)
    assert lib.ppo_obs_norm_freeze(ppo, 0) == 1
    # bad arguments: −1, the setting and the state unchanged
    assert lib.ppo_set_obs_norm(ppo, float("nan")) == -1 and lib.ppo_get_obs_norm(ppo) == 0.5
    bad_m2, bad_n, bad_nan = tri.copy(), tri.copy(), tri.copy()
    bad_m2[1 + S + 2], bad_n[0], bad_nan[2] = -1.0, -1.0, np.nan
    for bad in (bad_m2, bad_n, bad_nan, tri[:-1], np.concatenate([tri, [0.0]])):
        assert set_state(lib, ppo, bad) == -1
    np.testing.assert_array_equal(get_state(lib, ppo, S), tri)
    out = (C.c_double * (2 * S))()
    assert lib.ppo_obs_norm_get_state(ppo, out, 2 * S) == -1
    assert lib.ppo_obs_norm_affine(ppo, None, None, S + 1) == -1
    assert lib.ppo_obs_normalize_device(ppo, None, d.ptr, 8) == -1
    assert lib.ppo_obs_norm_freeze(ppo, 1) == 0 and lib.ppo_obs_norm_freeze(ppo, 0) == 1
    # turning it off keeps the state
    assert lib.ppo_set_obs_norm(ppo, 0.0) == 0 and lib.ppo_get_obs_norm(ppo) == 0.0
    np.testing.assert_array_equal(get_state(lib, ppo, S), tri)
    assert stats(lib, ppo, 19) == stats(lib, ppo)[:19]
    d.free()
    no_error(lib)
    lib.free_ppo(ppo)


# ----------------------------------------------------------------------------- 3. update == update on pre-normalised data
CONFIGS = {
    # name: (sizes, B, tiny path)
    "c3": ([17, 256, 256, 6], 1028, False),
    "fold": ([64, 256, 6], 2048, False),
    "tiny": ([3, 64, 64, 1], 64, True),
}


def raw_buffer(lib, ppo, N, S, seed):
    """A synthetic fill whose observations are then scaled and shifted per column on the host (state and
    next_state alike: bitwise-equal rows stay equal).  Returns (state, next_state)."""
    lib.ppo_fill_synthetic(ppo, 8, N // 8, 9, 1.0 / 200)
    lib.ppo_synchronize()
    b = ppo.contents.buffer.contents
    rng = np.random.default_rng(seed)
    scale = (10.0 ** rng.uniform(-1, 2, S)).astype(F32)
    shift = (scale * rng.uniform(-1, 1, S)).astype(F32)      # |mean| well inside 10·std: ordinary columns
    out = []
    for p in (b.d_state_p, b.d_next_state_p):
        x = (ppo_ffi.d2h(lib, p, F32, N * S).reshape(N, S) * scale + shift).astype(F32)
        ppo_ffi.h2d(lib, p, x)
        out.append(x)
    # a quarter of the columns get a running std four times too small: clip 5 clamps part of them
    std = scale.astype(np.float64) / np.sqrt(3.0) * np.where(np.arange(S) % 4 == 1, 0.25, 1.0)
    return out[0], out[1], known_triple(S, shift.astype(np.float64) * 1.01, std, n=3000.0)


def one_update(lib, oracle, sizes, B, N, tri, clip, pre=None):
    S = sizes[0]
    ppo = make_ppo(lib, oracle, sizes, N, seed=4242)
    state, nstate, tri0 = raw_buffer(lib, ppo, N, S, 5)
    b = ppo.contents.buffer.contents
    out = dict(ppo=ppo, state=state, nstate=nstate, tri0=tri0)
    if pre is not None:                                    # run B: the host-normalised buffer, feature off
        m, r = pre
        ppo_ffi.h2d(lib, b.d_state_p, normalize_f32(state, m, r, clip)[0])
        ppo_ffi.h2d(lib, b.d_next_state_p, normalize_f32(nstate, m, r, clip)[0])
    else:
        assert lib.ppo_set_obs_norm(ppo, clip) == 0
        assert set_state(lib, ppo, tri0 if tri is None else tri) == 0
        out["pair"] = dev_affine(lib, ppo, S)
    lib.ppo_set_step_limit(ppo, 1, 1)
    lib.ppo_reset_stats(ppo)
    oracle.srand(99)
    lib.ppo_update(ppo, 0.99, B, 1, 1, 1, SEED)
    lib.ppo_synchronize()
    no_error(lib)
    pol = ppo.contents.policy.contents
    # μ's last forward through the layer kernels: the policy step's B rows in the multi-launch loop; in the
    # single-workgroup path the phases run no layer kernel, so it is still the synthetic fill's N rows
    out["mu_forward_m"] = pol.mu.contents.cache_m_forward
    out.update(st=stats(lib, ppo), adv=ppo_ffi.d2h(lib, b.d_advantage_p, F32, N),
               tgt=ppo_ffi.d2h(lib, b.d_adv_target_p, F32, N), gV=nn_grads_packed(lib, ppo.contents.V),
               gmu=nn_grads_packed(lib, pol.mu), gls=ppo_ffi.d2h(lib, pol.d_log_std_grad, F32, sizes[-1]),
               buf_state=ppo_ffi.d2h(lib, b.d_state_p, F32, N * S).reshape(N, S),
               buf_nstate=ppo_ffi.d2h(lib, b.d_next_state_p, F32, N * S).reshape(N, S))
    return out


@pytest.mark.parametrize("cfg", sorted(CONFIGS))
def test_update_equals_prenormalised(lib, oracle, cfg, monkeypatch):
    sizes, B, tiny = CONFIGS[cfg]
    monkeypatch.delenv("PPO_NO_TINY", raising=False)
    N, S, clip = 2 * B, sizes[0], 5.0
    a = one_update(lib, oracle, sizes, B, N, None, clip)
    m, r = a["pair"]
    if not tiny:
        a["xV"] = nn_input_rows(lib, a["ppo"].contents.V, B)
        a["xmu"] = nn_input_rows(lib, a["ppo"].contents.policy.contents.mu, B)
    bb = one_update(lib, oracle, sizes, B, N, None, clip, pre=(m, r))
    try:
        np.testing.assert_array_equal(a["state"], bb["state"])            # the same raw rollout
        # the path the configuration is here for was the one taken, with the feature on as with it off
        assert a["mu_forward_m"] == bb["mu_forward_m"] == (N if tiny else B), (a["mu_forward_m"], bb["mu_forward_m"])
        assert a["st"][1] == 1 and a["st"][3] == 1
        if not tiny:
            for k, nn in (("xV", bb["ppo"].contents.V), ("xmu", bb["ppo"].contents.policy.contents.mu)):
                np.testing.assert_array_equal(a[k].view(np.uint32), nn_input_rows(lib, nn, B).view(np.uint32))
        for k in ("adv", "tgt"):
            np.testing.assert_array_equal(a[k].view(np.uint32), bb[k].view(np.uint32))
        assert_gemm_close(a["gV"], bb["gV"], B, f"{cfg}: value grads, feature on vs pre-normalised")
        assert_gemm_close(a["gmu"], bb["gmu"], B, f"{cfg}: policy grads, feature on vs pre-normalised")
        assert_gemm_close(a["gls"], bb["gls"], B, f"{cfg}: log-std grads, feature on vs pre-normalised")
        assert np.abs(bb["gV"]).max() > 0 and np.abs(bb["gmu"]).max() > 0
        # the caller's buffer is never written
        np.testing.assert_array_equal(a["buf_state"].view(np.uint32), a["state"].view(np.uint32))
        np.testing.assert_array_equal(a["buf_nstate"].view(np.uint32), a["nstate"].view(np.uint32))
        # counters and the folded state
        _, cl = normalize_f32(a["state"], m, r, clip)
        st = a["st"]
        print(f"{cfg}: clamped {int(st[20])} of {int(st[21])} (model {int(cl.sum())}), count {st[19]}")
        assert cl.sum() > 0 and st[20] == cl.sum() and st[21] == N * S and bb["st"][19:] == [0, 0, 0]
        want = chan(a["tri0"], stats64(a["state"]))
        got = get_state(lib, a["ppo"], S)
        check_triple(got, want, np.zeros(S, int), f"{cfg}: running state after the update")
        assert st[19] == want[0] == got[0]
        # a frozen repeat normalises and leaves the state as it is
        assert lib.ppo_obs_norm_freeze(a["ppo"], 1) == 0
        lib.ppo_update(a["ppo"], 0.99, B, 1, 1, 1, SEED)
        lib.ppo_synchronize()
        np.testing.assert_array_equal(get_state(lib, a["ppo"], S).view(np.uint64), got.view(np.uint64))
        assert stats(lib, a["ppo"])[21] == N * S
        no_error(lib)
    finally:
        for r_ in (a, bb):
            lib.ppo_set_step_limit(r_["ppo"], -1, -1)
            lib.free_ppo(r_["ppo"])


# ----------------------------------------------------------------------------- 4. fold order
def test_fold_order(lib, oracle, monkeypatch):
    """Normalise with the pair on entry, fold afterwards: from an empty state the first update's layer-0 rows
    are the raw rows, the second update's — same buffer — are normalised by the first buffer's statistics."""
    monkeypatch.delenv("PPO_NO_TINY", raising=False)
    sizes, B = [64, 256, 6], 2048
    N, S, clip = 2 * B, sizes[0], 5.0
    ppo = make_ppo(lib, oracle, sizes, N, seed=4242)
    assert lib.ppo_set_obs_norm(ppo, clip) == 0
    state, _, _ = raw_buffer(lib, ppo, N, S, 5)
    lib.ppo_set_step_limit(ppo, 1, 0)

    def rows_of(x):
        return sorted(r.tobytes() for r in np.ascontiguousarray(x, F32))

    lib.ppo_update(ppo, 0.99, B, 0, 1, 1, SEED)
    lib.ppo_synchronize()
    x1 = nn_input_rows(lib, ppo.contents.V, B)
    raw = set(rows_of(state))
    assert len(set(rows_of(x1))) == B and set(rows_of(x1)) <= raw
    m, r = dev_affine(lib, ppo, S)
    m_ref, r_ref = affine(stats64(state))
    # fp32 roundings of statistics that agree to 1e-10: at most the neighbouring float
    assert (np.abs(m.astype(np.float64) - m_ref) <= np.spacing(np.abs(m_ref))).all()
    assert (np.abs(r.astype(np.float64) - r_ref) <= np.spacing(r_ref)).all()
    assert stats(lib, ppo)[19] == N
    lib.ppo_update(ppo, 0.99, B, 0, 1, 1, SEED)
    lib.ppo_synchronize()
    x2 = nn_input_rows(lib, ppo.contents.V, B)
    normed = set(rows_of(normalize_f32(state, m, r, clip)[0]))
    assert len(set(rows_of(x2))) == B and set(rows_of(x2)) <= normed and not (set(rows_of(x2)) & raw)
    assert stats(lib, ppo)[19] == 2 * N
    no_error(lib)
    lib.ppo_set_step_limit(ppo, -1, -1)
    lib.free_ppo(ppo)


# ----------------------------------------------------------------------------- 5. device rollout
@pytest.mark.parametrize("sizes,kind,mean,std", [([17, 256, 256, 6], 1, 0.3, 0.4),
                                                 ([3, 64, 64, 1], 0, [0.2, -0.1, 0.5], [0.7, 0.6, 3.0])])
def test_rollout_samples_from_normalised(lib, oracle, sizes, kind, mean, std):
    E = T = 64
    N, S, A, clip = E * T, sizes[0], sizes[-1], 10.0
    ppo = test_gpu_rollout.make(lib, sizes, N)
    assert lib.ppo_set_obs_norm(ppo, clip) == 0
    assert set_state(lib, ppo, known_triple(S, mean, std)) == 0
    assert lib.ppo_obs_norm_freeze(ppo, 1) == 0
    m, r = dev_affine(lib, ppo, S)
    fills = [("rollout", lambda: lib.ppo_rollout_device(ppo, E, T, kind, 11))]
    if kind == 1:
        fills.append(("fill_synthetic", lambda: lib.ppo_fill_synthetic(ppo, E, T, 13, 1.0 / 200)))
    for what, fill in fills:
        fill()
        lib.ppo_synchronize()
        no_error(lib)
        buf = test_gpu_rollout.read_buffer(lib, ppo, N, S, A)
        if what == "rollout":
            test_gpu_rollout.check_structure(buf, E, T)
        normed = dict(buf, state=normalize_f32(buf["state"], m, r, clip)[0])
        test_gpu_rollout.check_logprob(lib, oracle, ppo, normed, sizes)
        with pytest.raises(AssertionError):                 # a control on the data: raw states do not explain them
            test_gpu_rollout.check_logprob(lib, oracle, ppo, buf, sizes)
    np.testing.assert_array_equal(get_state(lib, ppo, S), known_triple(S, mean, std))
    lib.free_ppo(ppo)


# ----------------------------------------------------------------------------- 6. with the other options and paths
def _options_run(lib, oracle, obs):
    sizes, N, B = [17, 64, 64, 6], 1024, 256
    S = sizes[0]
    ppo = make_ppo(lib, oracle, sizes, N, seed=1234)
    if obs:
        assert lib.ppo_set_obs_norm(ppo, 5.0) == 0
        assert set_state(lib, ppo, known_triple(S, 0.1 * np.random.default_rng(3).normal(size=S), 1.0)) == 0
    lib.ppo_fill_synthetic(ppo, 4, N // 4, 99, 1.0 / 500)
    assert lib.ppo_set_max_grad_norm(ppo, 0.5) == 0 and lib.ppo_set_target_kl(ppo, float("inf")) == 0
    assert lib.ppo_set_value_clip(ppo, 0.2) == 0
    lib.ppo_reset_stats(ppo)
    lib.ppo_update(ppo, 0.99, B, 1, 2, 1, SEED)
    lib.ppo_synchronize()
    no_error(lib)
    hist = (C.c_double * 8)()
    assert lib.ppo_kl_history(ppo, hist, 8) == N // B
    st = stats(lib, ppo)
    lib.free_ppo(ppo)
    return st, hist[0]


def test_with_other_options(lib, oracle, monkeypatch):
    monkeypatch.setenv("PPO_NO_TINY", "1")
    st_off, kl_off = _options_run(lib, oracle, False)
    st_on, kl_on = _options_run(lib, oracle, True)
    print(f"kl_history[0]: obs-norm on {kl_on:.6g}, off {kl_off:.6g}")
    assert np.isfinite(st_on).all() and np.isfinite(st_off).all()
    assert st_on[1] == 8 and st_on[3] == 4 and st_on[18] == 2 * 1024 and st_on[15] == 4
    assert st_on[19] == 5000 + 1024 and st_on[21] == 1024 * 17 and st_off[19:] == [0, 0, 0]
    # the first policy step sees the policy that sampled the buffer: its KL is rounding, as with the feature off
    assert 0 <= kl_on <= 4 * kl_off


def test_graph_replay(lib, oracle, monkeypatch):
    """The feature keeps graph replay available (test_gpu_update.test_graph_replay_matches_eager's shape)."""
    sizes, N, B = [17, 256, 256, 6], 1024, 64
    S = sizes[0]
    monkeypatch.setenv("PPO_NO_CLUSTER", "1")
    out = {}
    for mode in ("eager", "graph"):
        if mode == "eager":
            monkeypatch.delenv("PPO_GRAPH", raising=False)
        else:
            monkeypatch.setenv("PPO_GRAPH", "1")
            monkeypatch.setenv("PPO_GRAPH_STEPS", "16")
        ppo = make_ppo(lib, oracle, sizes, N, init_std=0.7, ent_coeff=0.01)
        assert lib.ppo_set_obs_norm(ppo, 5.0) == 0
        assert set_state(lib, ppo, known_triple(S, 0.2, 0.5)) == 0
        lib.ppo_fill_synthetic(ppo, 8, N // 8, 44, 1.0 / 200)
        lib.ppo_reset_stats(ppo)
        lib.ppo_update(ppo, 0.99, B, 1, 2, 1, SEED)
        lib.ppo_synchronize()
        no_error(lib)
        pol = ppo.contents.policy.contents
        out[mode] = dict(st=stats(lib, ppo), v=nn_params_packed(lib, ppo.contents.V), mu=nn_params_packed(lib, pol.mu))
        lib.free_ppo(ppo)
    a, b = out["eager"], out["graph"]
    assert a["st"][8] == 0 and b["st"][8] > 0, b["st"][8]
    assert b["st"][21] == N * S and b["st"][19] == 5000 + N
    assert_gemm_close(b["v"], a["v"], B, "value parameters, graph replay vs eager")
    assert_gemm_close(b["mu"], a["mu"], B, "policy parameters, graph replay vs eager")


# ----------------------------------------------------------------------------- 7. data parallelism in loopback
def test_loopback_fold_and_hash(lib, oracle, monkeypatch):
    sizes, N, B = [17, 64, 64, 6], 1024, 256
    S = sizes[0]
    monkeypatch.setenv("PPO_COMM_LOOPBACK", "2")
    assert lib.ppo_comm_init(0, 1, None) == 0, lib.ppo_last_error()
    try:
        assert lib.ppo_comm_world() == 2
        ppo = make_ppo(lib, oracle, sizes, N, seed=1234)
        assert lib.ppo_set_obs_norm(ppo, 5.0) == 0
        lib.ppo_fill_synthetic(ppo, 4, N // 4, 99, 1.0 / 500)
        out = (C.c_double * (1 + 2 * S))()
        assert lib.ppo_obs_stats_device(ppo.contents.buffer.contents.d_state_p, N, S, out) == 0
        one = np.array(out[:])
        lib.ppo_set_step_limit(ppo, 1, 1)
        lib.ppo_update(ppo, 0.99, B, 1, 1, 1, SEED)
        lib.ppo_synchronize()                              # returns: no collective left waiting
        no_error(lib)
        got = get_state(lib, ppo, S)
        assert got[0] == 2 * N and stats(lib, ppo)[19] == 2 * N
        np.testing.assert_allclose(got[1:1 + S], one[1:1 + S], rtol=1e-12, atol=0)
        np.testing.assert_allclose(got[1 + S:], 2 * one[1 + S:], rtol=1e-12, atol=0)
        lib.ppo_set_step_limit(ppo, -1, -1)
        lib.free_ppo(ppo)
    finally:
        lib.ppo_comm_finalize()
        monkeypatch.delenv("PPO_COMM_LOOPBACK")
    # the hash covers the state while the feature is on, and only then
    p1, p2 = (make_ppo(lib, oracle, sizes, N, seed=1234) for _ in range(2))
    assert lib.ppo_param_hash(p1) == lib.ppo_param_hash(p2)
    h_off = lib.ppo_param_hash(p1)
    # a function of the state only: on and never touched hashes like on and set to the empty state
    assert lib.ppo_set_obs_norm(p1, 5.0) == 0 and lib.ppo_set_obs_norm(p2, 5.0) == 0
    assert set_state(lib, p2, np.zeros(1 + 2 * S)) == 0
    assert lib.ppo_param_hash(p1) == lib.ppo_param_hash(p2) != h_off
    for p, mean in ((p1, 0.25), (p2, 0.5)):
        assert lib.ppo_set_obs_norm(p, 5.0) == 0 and set_state(lib, p, known_triple(S, mean, 1.0)) == 0
    assert lib.ppo_param_hash(p1) != lib.ppo_param_hash(p2)
    assert set_state(lib, p2, known_triple(S, 0.25, 1.0)) == 0
    assert lib.ppo_param_hash(p1) == lib.ppo_param_hash(p2) != h_off
    for p in (p1, p2):
        assert lib.ppo_set_obs_norm(p, 0.0) == 0
    assert lib.ppo_param_hash(p1) == lib.ppo_param_hash(p2) == h_off
    lib.free_ppo(p1)
    lib.free_ppo(p2)
