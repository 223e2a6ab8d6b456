"""Which front end an MSM launch takes is a pure function of its shape (engine.h msm_dense_front_applies, through
`mg_msm_dense_front_applies`): one scalar vector over one query, window tables of at most 16 windows, no compaction asked for.
No GPU: the function touches no device, and `mg_msm_dense_front` refuses a shape it turns down before any device work."""
import ctypes

import numpy as np

from manta_rs_amd import api


def test_the_path_is_decided_by_batch_queries_windows_tables_and_sparse():
    for batch in (1, 2, 32):
        for n_sets in (1, 2, 3):
            for W in (0, 1, 15, 16, 17, 32, 127):
                for table_mode in (0, 1, 2):  # plain bases, window tables, full tables
                    for sparse in (False, True):
                        want = batch == 1 and n_sets == 1 and 1 <= W <= 16 and table_mode == 1 and not sparse
                        assert api.msm_dense_front_applies(batch, n_sets, W, table_mode, sparse) == want, (batch, n_sets, W, table_mode, sparse)
    # the headline: 2^20 BLS12-381 scalars on 17-bit tables, 15 windows; one bit narrower is 17 windows and not dense
    assert api.msm_dense_front_applies(1, 1, (255 + 16) // 17, 1, False) and not api.msm_dense_front_applies(1, 1, (255 + 14) // 15, 1, False)
    assert not api.msm_dense_front_applies(1 << 40, 1, 15, 1, False)  # (no wrap into 32 bits)


def test_the_fused_entry_point_refuses_a_shape_that_is_not_dense_before_any_device_work():
    sz, u32 = ctypes.c_size_t, ctypes.c_uint32
    sc = np.ones((2, 4), dtype=np.uint64)
    buf = np.zeros(64, dtype=np.uint32)
    layout = (u32 * 4)()

    def front(curve=0, scalars=sc, n_scalars=2, flags=0, c=16, n=2, map=None, set_len=2, keys=buf, vals=buf, lay=layout):
        return api.LIB.mg_msm_dense_front(curve, api._p(scalars), sz(n_scalars), flags, c, sz(n), api._p(map), sz(set_len), api._p(keys),
                                          api._p(vals), lay)

    refused = dict(curve=front(curve=2), no_scalars=front(scalars=None), no_keys=front(keys=None), no_vals=front(vals=None), no_layout=front(lay=None),
                   flags=front(flags=2), c0=front(c=0), c25=front(c=25), seventeen_windows=front(c=15), bls_seventeen_windows=front(curve=1, c=15),
                   n0=front(n=0, set_len=0), no_scalar=front(n_scalars=0), n_is_not_the_set=front(n=2, set_len=3), scalars_beyond_the_set=front(n_scalars=3),
                   map_entry_beyond_the_set=front(map=np.array([0, 4], dtype=np.uint32), set_len=3),
                   # 16 windows x 2^27 bases: the infinity record's index would be 2^31
                   base_index=front(n=1 << 27, set_len=1 << 27))
    assert refused == {k: 1 for k in refused}, refused
