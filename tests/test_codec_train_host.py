"""Codec training, the parts that need no device: the restated order-free sum (tests/codec_train_ref.py) against float64 and against its
own definition, opq_msgpack, and the argument refusals of the mse_pq_trainer ABI (include/mse.h)."""
import ctypes as C

import numpy as np
import pytest

import codec_train_ref as ref


@pytest.mark.parametrize("n,w,n_cells", [(1, 18, 7), (63, 36, 7), (1000, 18, 256), (4133, 5, 3)])
def test_restated_sum_is_close_to_float64_and_order_free(n, w, n_cells):
    """Each term is rounded to a multiple of 2^-E, half a unit at most: a cell of n rows is within n 2^-(E+1) of the float64 sum (whose
    own error, n 2^-53 of the absolute sum, is far below that here).  Integer adds commute: any row order gives the same int64."""
    rng = np.random.default_rng(n * 7 + w)
    v = (rng.standard_normal((n, w)) * 2.0 ** rng.integers(-20, 1, (n, 1))).astype(np.float32)
    code = rng.integers(0, n_cells, n).astype(np.uint8)
    S, E = ref.accumulate_by_code(v, code, n_cells)
    exact = np.zeros((n_cells, w), np.float64)
    np.add.at(exact, code, v.astype(np.float64))
    assert np.all(np.abs(S.astype(np.float64) * 2.0 ** -E - exact) <= n * 2.0 ** -(E + 1))
    assert np.abs(S).max() < 2 ** 61
    perm = rng.permutation(n)
    S2, E2 = ref.accumulate_by_code(v[perm], code[perm], n_cells)
    assert E2 == E and np.array_equal(S, S2)


def test_exponent_rule_at_its_edges():
    """vmax = f 2^ex with f in [0.5, 1): an exact power of two 2^p has ex = p + 1; n an exact power of two has ceil(log2 n) = log2 n and
    n + 1 the next integer; an all-zero input takes ex = 0."""
    assert ref.fixed_exponent(1.0, 1) == 61 - 0 - 1
    assert ref.fixed_exponent(0.99999994, 1) == 61 - 0 - 0
    assert ref.fixed_exponent(2.0 ** -20, 1) == 61 + 19
    assert ref.fixed_exponent(np.nextafter(np.float32(2.0 ** -20), np.float32(0)), 1) == 61 + 20
    assert ref.fixed_exponent(0.75, 1024) == 61 - 10
    assert ref.fixed_exponent(0.75, 1025) == 61 - 11
    assert ref.fixed_exponent(0.75, 2) == 61 - 1
    assert ref.fixed_exponent(0.0, 1000) == 61 - 10
    assert ref.fixed_exponent(2.0 ** -149, 1) == 61 + 148       # the smallest subnormal
    S, E = ref.accumulate_by_code(np.zeros((5, 3), np.float32), np.zeros(5, np.uint8), 2)
    assert E == 61 - 3 and not S.any()
    # the largest term stays below 2^(61 - ceil(log2 n)): n of them fit int64 with room to spare
    for vmax, n in [(1.0, 4096), (0.99999994, 4097), (3.0e38, 7)]:
        E = ref.fixed_exponent(vmax, n)
        assert abs(np.rint(np.ldexp(np.float64(np.float32(vmax)), E))) * n <= 2.0 ** 61
    with pytest.raises(ValueError):
        ref.accumulate_by_code(np.array([[np.inf]], np.float32), np.zeros(1, np.uint8), 1)


def test_opq_msgpack_round_trip(mse):
    import msgpack
    rng = np.random.default_rng(0)
    cent = rng.standard_normal((5, 12)).astype(np.float32)
    T = rng.standard_normal((12, 12)).astype(np.float32)
    blob = mse.opq_msgpack(cent, T, 4, 12)
    m = msgpack.unpackb(blob, raw=False)
    assert sorted(m) == ["centroids", "n_dims", "n_dims_per_code", "transform"]
    assert m["n_dims"] == 12 and m["n_dims_per_code"] == 4
    assert isinstance(m["centroids"], list) and len(m["centroids"]) == 60 and len(m["transform"]) == 144
    assert np.array_equal(np.asarray(m["centroids"], np.float32), cent.reshape(-1))       # f32 -> f64 list -> f32 is exact
    assert np.array_equal(np.asarray(m["transform"], np.float32), T.reshape(-1))
    with pytest.raises(mse.MseError):
        mse.opq_msgpack(cent, T[:, :11], 4, 12)


def test_trainer_refuses_bad_arguments_without_a_device(mse):
    from mse import ffi
    L = ffi.lib()
    assert not L.mse_pq_trainer_new(1152, 18, 257)
    assert "256" in ffi.last_error()
    assert not L.mse_pq_trainer_new(1152, 18, 0)
    assert not L.mse_pq_trainer_new(1152, 17, 256)
    assert "multiple" in ffi.last_error()
    assert not L.mse_pq_trainer_new(0, 18, 256)
    x = np.zeros(4, np.float32)
    out = C.c_double(0.0)
    for rc in (L.mse_pq_trainer_set_sample_f32(None, x.ctypes.data_as(ffi.f32p), 1),
               L.mse_pq_trainer_set_sample_base(None, None, None, 0),
               L.mse_pq_trainer_set_transform(None, x.ctypes.data_as(ffi.f32p)),
               L.mse_pq_trainer_set_centroids(None, x.ctypes.data_as(ffi.f32p)),
               L.mse_pq_trainer_set_query_moment(None, x.ctypes.data_as(ffi.f32p)),
               L.mse_pq_trainer_kmeans(None, 1, None),
               L.mse_pq_trainer_refine(None, 1, 1e-3, 0.9, 0.999, 1e-8, C.byref(out)),
               L.mse_pq_trainer_loss(None, C.byref(out)),
               L.mse_pq_trainer_cross(None, C.byref(out)),
               L.mse_pq_trainer_read(None, None, None),
               L.mse_pq_trainer_codes(None, None),
               L.mse_pq_trainer_adam_state(None, None, None, None),
               L.mse_pq_trainer_timing(None, None)):
        assert rc != 0 and "null trainer" in ffi.last_error()
    assert not L.mse_pq_trainer_finish(None)
    assert "null trainer" in ffi.last_error()
    L.mse_pq_trainer_free(None)
    # the test hooks check their shapes before any device work
    s = np.zeros(4, np.int64)
    e = C.c_int(0)
    code = np.zeros(1, np.uint8)
    assert L.mse_debug_accumulate_by_code(x.ctypes.data_as(ffi.f32p), 1, 4, code.ctypes.data_as(ffi.u8p), 257, s.ctypes.data_as(ffi.i64p), C.byref(e)) != 0
    assert "cells" in ffi.last_error()
    code[0] = 3
    assert L.mse_debug_accumulate_by_code(x.ctypes.data_as(ffi.f32p), 1, 4, code.ctypes.data_as(ffi.u8p), 2, s.ctypes.data_as(ffi.i64p), C.byref(e)) != 0
    assert "n_cells" in ffi.last_error()
    with pytest.raises(mse.MseError):
        mse.CodecTrainer(1152, 18, 300)
