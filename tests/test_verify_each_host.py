"""The chunk of the per-item verification calls is one number in three places (mantagpu.h, api.py, mantagpu-sys), and the
argument checks of the Python wrappers that refuse a call before it reaches the library need no GPU."""
import os
import re

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


def test_chunk_is_one_number_everywhere():
    from manta_rs_amd import api
    hdr = open(os.path.join(HERE, "..", "include", "mantagpu.h")).read()
    rs = open(os.path.join(HERE, "..", "rust", "mantagpu-sys", "src", "lib.rs")).read()
    c = int(re.search(r"#define MG_VERIFY_EACH_CHUNK (\d+)u", hdr).group(1))
    assert c == api.VERIFY_EACH_CHUNK == int(re.search(r"pub const MG_VERIFY_EACH_CHUNK: usize = (\d+);", rs).group(1))
    assert c & (c - 1) == 0 and c <= 4096, "a power of two no larger than 4 096"
    assert c <= 65535, "a chunk is one batched MSM launch: at most 65 535 scalar vectors"


def test_pairing_check_each_refuses_mismatched_shapes():
    from manta_rs_amd import api
    w1, w2 = api.affine_limbs(0, 1), api.affine_limbs(0, 2)
    g1, g2 = np.zeros((3, 2, w1), np.uint64), np.zeros((3, 2, w2), np.uint64)
    for a, b in ((g1, g2[:2]), (g1, g2[:, :1]), (g1.reshape(6, w1), g2.reshape(6, w2)), (g1[:, :, :-1], g2)):
        with pytest.raises(ValueError):
            api.pairing_check_each(0, a, b)
    with pytest.raises(ValueError):
        api.pairing_check_each(0, g1, g2, out=np.zeros(2, np.uint8))
