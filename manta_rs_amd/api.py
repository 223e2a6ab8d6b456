"""ctypes binding of libmantagpu.so + the Python mirror of the reference's prover interface.

Every call goes through the C ABI declared in include/mantagpu.h -- the same entry points the Rust
shim of INTEGRATION.md binds. There is no CPU path here: if the shared library (built by
`__graft_entry__.build()` / `make -C manta_rs_amd/csrc`) is absent, import raises.
"""
from __future__ import annotations

import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MANTA_LIB") or os.path.join(_HERE, "lib", "libmantagpu.so")  # MANTA_LIB: A/B builds only

BN254, BLS12_381 = 0, 1
FQ_LIMBS = {BN254: 4, BLS12_381: 6}


class MantaGpuError(RuntimeError):
    """Mirror of the reference's opaque unit `Error` (manta-crypto/src/arkworks/groth16.rs:50-60),
    carrying the status code and the library's detail string."""

    def __init__(self, status, where=""):
        self.status = status
        detail = LIB.mg_last_error().decode() if status == 2 else ""
        super().__init__(f"{where}: {LIB.mg_strerror(status).decode()} ({status}) {detail}")


# The C ABI's types, stated here and nowhere else: "return:parameters" per entry point of include/mantagpu.h, in the header's
# order (tests/test_host.py parses the header and holds this table to it). Letters: i int / mg_curve_t, u unsigned / uint32_t,
# z size_t, q uint64_t, f float, v void, s const char * returned, n mg_tuning_env_names' list, p any pointer, array or handle.
# ctypes converts by these, so a count of 2^32 + 5 arrives as that and not as 5; it checks no range: the wrappers do.
_KINDS = {"i": ctypes.c_int, "u": ctypes.c_uint32, "z": ctypes.c_size_t, "q": ctypes.c_uint64, "f": ctypes.c_float, "v": None,
          "s": ctypes.c_char_p, "n": ctypes.POINTER(ctypes.c_char_p), "p": ctypes.c_void_p}
_SIGNATURES = {
    "mg_init": "i:i",
    "mg_strerror": "s:i",
    "mg_last_error": "s:",
    "mg_device_count": "i:p",
    "mg_malloc": "i:pz",
    "mg_free": "i:p",
    "mg_memcpy_h2d": "i:ppz",
    "mg_memcpy_d2h": "i:ppz",
    "mg_device_synchronize": "i:",
    "mg_host_alloc": "i:pz",
    "mg_host_free": "i:p",
    "mg_set_kernel_timing": "i:i",
    "mg_last_accumulate_ms": "f:",
    "mg_last_accumulate_mhz": "f:",
    "mg_clock_probe": "i:uppp",
    "mg_last_ntt_ms": "i:p",
    "mg_last_prove_phases_ms": "i:p",
    "mg_last_pass_host_ms": "i:p",
    "mg_hw_queues": "i:p",
    "mg_bases_create": "i:iipziip",
    "mg_bases_create_sharded": "i:iipzpiip",
    "mg_bases_num_shards": "i:p",
    "mg_bases_shard": "i:pippp",
    "mg_bases_destroy": "v:p",
    "mg_bases_device_bytes": "z:p",
    "mg_msm": "i:ppzp",
    "mg_msm_launch": "i:ppziip",
    "mg_msm_launch_sharded": "i:ppiip",
    "mg_msm_finish": "i:pp",
    "mg_msm_result_to_device": "i:ppp",
    "mg_xyzz_limbs": "z:ii",
    "mg_xyzz_sum": "i:iipzp",
    "mg_points_sum": "i:iipzp",
    "mg_fixed_base_mul": "i:iippzp",
    "mg_ec_elementwise": "i:iiippzp",
    "mg_field_op": "i:iiiiippzp",
    "mg_fpr_raw_op": "i:iiippppzp",
    "mg_fpr_column_plan": "i:iippppp",
    "mg_msm_digits": "i:ipzziiizpzzipppp",
    "mg_sort_pairs": "i:ppzipuupp",
    "mg_msm_dense_front_applies": "i:zziii",
    "mg_msm_dense_front": "i:ipziizpzppp",
    "mg_group_ntt": "i:iipuip",
    "mg_point_serialize": "i:iipip",
    "mg_ntt": "i:ipuii",
    "mg_ntt_device": "i:ipuii",
    "mg_groth16_setup": "i:ipppqqqpppp",
    "mg_qap_columns": "i:iizppqqup",
    "mg_mpc_initialize": "i:ippppqqqqppp",
    "mg_ctx_create": "i:ipp",
    "mg_tuning_init": "i:p",
    "mg_get_tuning": "i:p",
    "mg_set_tuning": "i:p",
    "mg_tuning_env_names": "n:",
    "mg_ctx_opts_init": "i:p",
    "mg_ctx_create_ex": "i:ippp",
    "mg_ctx_create_from_bytes_ex": "i:ipzppp",
    "mg_ctx_create_sharded": "i:ippip",
    "mg_ctx_create_from_bytes_sharded": "i:ipzpip",
    "mg_ctx_create_shard": "i:ipiip",
    "mg_ctx_create_task": "i:ipup",
    "mg_partials_slot_limbs": "z:p",
    "mg_groth16_partials_launch": "i:pqpppp",
    "mg_groth16_partials_finish": "i:p",
    "mg_groth16_assemble": "i:pqipppp",
    "mg_ctx_create_from_bytes": "i:ipzp",
    "mg_ctx_create_from_bytes_checked": "i:ipzpp",
    "mg_blake3": "i:pzp",
    "mg_blake2s256": "i:pzp",
    "mg_blake2s": "i:pzzp",
    "mg_aes256_gcm": "i:pppzipp",
    "mg_ctx_set_r1cs": "i:ppppq",
    "mg_groth16_prove": "i:ppppp",
    "mg_groth16_prove_batch": "i:pqpppp",
    "mg_witness_map": "i:ppp",
    "mg_ctx_r1cs_check": "i:pqppp",
    "mg_r1cs_check": "i:ipppqqqppp",
    "mg_ctx_domain_size": "q:p",
    "mg_ctx_table_bytes": "i:pp",
    "mg_ctx_num_variables": "q:p",
    "mg_ctx_num_inputs": "q:p",
    "mg_ctx_num_shards": "i:p",
    "mg_ctx_destroy": "v:p",
    "mg_vk_create": "i:ipppppqp",
    "mg_vk_create_from_bytes": "i:ipzp",
    "mg_vk_encoded_size": "z:p",
    "mg_vk_encode": "i:pp",
    "mg_vk_alpha_beta": "i:pp",
    "mg_vk_num_inputs": "q:p",
    "mg_vk_destroy": "v:p",
    "mg_groth16_verify": "i:pppp",
    "mg_groth16_verify_batch": "i:pqpppp",
    "mg_pairing_check_each": "i:ippzzp",
    "mg_groth16_verify_each": "i:pqppp",
    "mg_pairing_check": "i:ippzp",
    "mg_pairing_op": "i:iipppzp",
    "mg_proof_decode": "i:ipp",
    "mg_points_decode": "i:iipziippp",
    "mg_points_check": "i:iipzpp",
    "mg_points_encode": "i:iipzip",
    "mg_proofs_decode": "i:ipzpp",
    "mg_ppot_points_decode": "i:iipziippp",
    "mg_ppot_points_encode": "i:iipzip",
    "mg_blake2b512": "i:pzp",
    "mg_poseidon_create": "i:iiiipzp",
    "mg_poseidon_destroy": "v:p",
    "mg_poseidon_permute": "i:ppz",
    "mg_poseidon_hash": "i:ppzp",
    "mg_poseidon_hash_device": "i:ppzp",
    "mg_merkle_tree": "i:pupzppzp",
    "mg_merkle_forest_roots": "i:puppzp",
    "mg_merkle_forest_append": "i:puzpppppppzpppzp",
    "mg_edwards_decode": "i:ipzippp",
    "mg_edwards_encode": "i:ipzp",
    "mg_edwards_check": "i:ipzpp",
    "mg_edwards_mul": "i:iipzpzp",
    "mg_edwards_add": "i:ippzp",
    "mg_note_cipher_create": "i:ipzpp",
    "mg_note_cipher_destroy": "v:p",
    "mg_notes_encrypt": "i:ppppzppp",
    "mg_notes_decrypt": "i:pppppzppp",
    "mg_utxo_model_create": "i:ipp",
    "mg_utxo_model_destroy": "v:p",
    "mg_utxos_mint": "i:ppppzppp",
    "mg_utxos_open": "i:pppppzpppp",
    "mg_viewing_keys": "i:ppzpp",
    "mg_schnorr_challenges": "i:ppppzpzp",
    "mg_signatures_verify": "i:pppppzpzpp",
    "mg_signatures_sign": "i:ppppzpzppp",
    "mg_address_partitions": "i:ppzp",
    "mg_merkle_shard_indices": "i:ipzp",
    "mg_light_notes_encrypt": "i:ppppzppp",
    "mg_light_notes_open": "i:pppppzpppp",
    "mg_outgoing_notes_encrypt": "i:ppppzppp",
    "mg_outgoing_notes_open": "i:ppppzppp",
}
EXPORTS = list(_SIGNATURES)


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} not found: the MI355X HIP library is the product and there is no CPU fallback. "
            "Run `python -c 'import __graft_entry__ as g; g.build()'` (or `make -C manta_rs_amd/csrc`).")
    try:  # share torch's HIP runtime if torch is (or will be) in this process
        import torch  # noqa: F401
    except Exception:  # pragma: no cover
        pass
    lib = ctypes.CDLL(LIB_PATH, mode=ctypes.RTLD_GLOBAL)
    for name, sig in _SIGNATURES.items():
        ret, params = sig.split(":")
        fn = getattr(lib, name)  # a symbol the library lacks fails the import here
        fn.restype, fn.argtypes = _KINDS[ret], [_KINDS[k] for k in params]
    return lib


LIB = _load()
_vp = ctypes.c_void_p
_sz = ctypes.c_size_t


def _chk(rc, where):
    if rc != 0:
        raise MantaGpuError(rc, where)


def _p(a):
    return None if a is None else a.ctypes.data_as(_vp)


def _u64(a):
    return np.ascontiguousarray(a, dtype=np.uint64)


def _addr(x):
    """a device / stream address given as int, ctypes.c_void_p or DeviceBuffer -> c_void_p"""
    if x is None:
        return None
    if isinstance(x, ctypes.c_void_p):
        return x
    if hasattr(x, "ptr"):
        return _addr(x.ptr)
    return _vp(int(x))


def init(device=0):
    _chk(LIB.mg_init(device), "mg_init")


def device_count():
    c = ctypes.c_int(0)
    _chk(LIB.mg_device_count(ctypes.byref(c)), "mg_device_count")
    return c.value


def set_kernel_timing(on):
    _chk(LIB.mg_set_kernel_timing(bool(on)), "mg_set_kernel_timing")


def last_accumulate_ms():
    return float(LIB.mg_last_accumulate_ms())


def last_accumulate_mhz():
    return float(LIB.mg_last_accumulate_mhz())


def clock_probe(iters=200000):
    """`mg_clock_probe`: (MHz the s_memtime counter ran at, wave-level v_mad_u64_u32 issued per SIMD and microsecond, probe ms)
    under an all-SIMD integer multiply-add load of two wavefronts per SIMD"""
    a, b, c = ctypes.c_double(0), ctypes.c_double(0), ctypes.c_double(0)
    _chk(LIB.mg_clock_probe(iters, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)), "mg_clock_probe")
    return a.value, b.value, c.value


def last_ntt_ms():
    """with kernel timing on: (whole call, conversion in, butterfly passes, conversion out) of this thread's last NTT, ms"""
    v = (ctypes.c_float * 4)()
    _chk(LIB.mg_last_ntt_ms(v), "mg_last_ntt_ms")
    return [float(x) for x in v]


def hw_queues():
    """(normal-priority, high-priority) hardware queues the library found behind the current device's streams; (0, 0) before the
    first ProvingContext of the process or with MANTA_QUEUE_AWARE=0 (mantagpu.h mg_hw_queues)"""
    v = (ctypes.c_int * 2)()
    _chk(LIB.mg_hw_queues(v), "mg_hw_queues")
    return int(v[0]), int(v[1])


def last_prove_phases_ms():
    """with kernel timing on: the phase split of this thread's last single proof (see mantagpu.h), ms"""
    v = (ctypes.c_float * 10)()
    _chk(LIB.mg_last_prove_phases_ms(v), "mg_last_prove_phases_ms")
    names = ("upload_z", "witness_map", "msm_a", "msm_b_g1", "msm_b_g2", "msm_l", "msm_h", "part_a_upload_to_join", "g2_chain_upload_to_end",
             "host_assembly_after_gpu")
    return {n: round(float(x), 4) for n, x in zip(names, v)}


def last_pass_host_ms():
    """host side of this thread's last proving pass: ms spent enqueuing, waiting for the GPU, assembling (`mg_last_pass_host_ms`)"""
    v = (ctypes.c_float * 3)()
    _chk(LIB.mg_last_pass_host_ms(v), "mg_last_pass_host_ms")
    return {"enqueue": round(float(v[0]), 4), "wait_gpu": round(float(v[1]), 4), "assemble": round(float(v[2]), 4)}


def synchronize():
    _chk(LIB.mg_device_synchronize(), "mg_device_synchronize")


class PinnedArray:
    """A numpy array in page-locked host memory (`mg_host_alloc`): assignments kept in one are uploaded to the GPU
    without the library's staging copy. `PinnedArray.like(arr).array` is a pinned copy of `arr`."""

    def __init__(self, shape, dtype=np.uint64):
        self.nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
        ptr = _vp()
        _chk(LIB.mg_host_alloc(ctypes.byref(ptr), self.nbytes), "mg_host_alloc")
        self._ptr = ptr
        buf = (ctypes.c_uint8 * self.nbytes).from_address(ptr.value)
        self.array = np.frombuffer(buf, dtype=dtype).reshape(shape)

    @classmethod
    def like(cls, arr):
        arr = np.ascontiguousarray(arr)
        p = cls(arr.shape, arr.dtype)
        p.array[...] = arr
        return p

    def free(self):
        if self._ptr is not None and self._ptr.value:
            self.array = None
            LIB.mg_host_free(self._ptr)
            self._ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class DeviceBuffer:
    """A raw HBM allocation owned by the library's HIP runtime."""

    def __init__(self, nbytes):
        self.nbytes = int(nbytes)
        ptr = _vp()
        _chk(LIB.mg_malloc(ctypes.byref(ptr), self.nbytes), "mg_malloc")
        self.ptr = ptr

    @classmethod
    def from_numpy(cls, arr):
        arr = np.ascontiguousarray(arr)
        b = cls(arr.nbytes)
        _chk(LIB.mg_memcpy_h2d(b.ptr, _p(arr), arr.nbytes), "mg_memcpy_h2d")
        return b

    def to_numpy(self, dtype=np.uint64, shape=None):
        out = np.empty(self.nbytes // np.dtype(dtype).itemsize, dtype=dtype)
        _chk(LIB.mg_memcpy_d2h(_p(out), self.ptr, self.nbytes), "mg_memcpy_d2h")
        return out if shape is None else out.reshape(shape)

    def offset(self, nbytes):
        return _vp(self.ptr.value + int(nbytes))

    def free(self):
        if self.ptr is not None and self.ptr.value:
            LIB.mg_free(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def affine_limbs(curve, group):
    return 2 * FQ_LIMBS[curve] * (2 if group == 2 else 1)


class Bases:
    """A static vector of curve points resident in HBM (the `bases: &[G::Affine]` argument of
    `VariableBaseMSM::multi_scalar_mul`, made persistent because proving-key queries never change)."""

    def __init__(self, curve, group, points, precompute_window_bits=0, on_device=False, devices=None):
        """devices: a list of HIP device indices -> the vector is range-sharded over them (`mg_bases_create_sharded`;
        a device may repeat); None -> one shard on the current device."""
        self.curve, self.group = curve, group
        h = _vp()
        if devices is not None:
            pts = _u64(points)
            assert pts.ndim == 2 and pts.shape[1] == affine_limbs(curve, group), pts.shape
            self.n = pts.shape[0]
            dv = (ctypes.c_int * len(devices))(*devices)
            _chk(LIB.mg_bases_create_sharded(curve, group, _p(pts), self.n, dv, len(devices), precompute_window_bits,
                                             ctypes.byref(h)), "mg_bases_create_sharded")
        elif on_device:
            ptr, n = points
            _chk(LIB.mg_bases_create(curve, group, ptr, n, 1, precompute_window_bits, ctypes.byref(h)), "mg_bases_create")
            self.n = n
        else:
            pts = _u64(points)
            assert pts.ndim == 2 and pts.shape[1] == affine_limbs(curve, group), pts.shape
            self.n = pts.shape[0]
            _chk(LIB.mg_bases_create(curve, group, _p(pts), self.n, 0, precompute_window_bits, ctypes.byref(h)), "mg_bases_create")
        self.handle = h
        self.precompute_window_bits = int(precompute_window_bits)

    def device_bytes(self):
        return LIB.mg_bases_device_bytes(self.handle)

    def shards(self):
        """[(device, lo, hi)] of the range shards."""
        out = []
        for g in range(LIB.mg_bases_num_shards(self.handle)):
            dev, lo, hi = ctypes.c_int(0), _sz(0), _sz(0)
            _chk(LIB.mg_bases_shard(self.handle, g, ctypes.byref(dev), ctypes.byref(lo), ctypes.byref(hi)), "mg_bases_shard")
            out.append((dev.value, lo.value, hi.value))
        return out

    def close(self):
        if self.handle is not None:
            LIB.mg_bases_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class MsmJob:
    def __init__(self, bases, handle):
        self.bases, self.handle = bases, handle

    def finish(self):
        out = np.zeros(affine_limbs(self.bases.curve, self.bases.group), dtype=np.uint64)
        _chk(LIB.mg_msm_finish(self.handle, _p(out)), "mg_msm_finish")
        self.handle = None
        return out

    def result_to_device(self, d_out_ptr, stream=None):
        """`mg_msm_result_to_device`: the window sums are folded on the GPU and the XYZZ result is written to device memory
        at d_out_ptr (xyzz_limbs u64); `stream` (raw hipStream_t as int, e.g. torch.cuda.current_stream().cuda_stream; None or
        0 = the default stream) is made to wait for it. No host synchronisation. The job must still be released with release()."""
        _chk(LIB.mg_msm_result_to_device(self.handle, _addr(d_out_ptr), _addr(stream)), "mg_msm_result_to_device")

    def release(self):
        """waits for the job and frees it without converting the result (its consumer took it on the device)"""
        _chk(LIB.mg_msm_finish(self.handle, None), "mg_msm_finish")
        self.handle = None


class VariableBaseMSM:
    """Mirror of ark_ec::msm::VariableBaseMSM (ark-ec 0.3.0; call sites in ark-groth16 create_proof,
    reached from manta-crypto/src/arkworks/groth16.rs:597)."""

    @staticmethod
    def multi_scalar_mul(bases: Bases, scalars) -> np.ndarray:
        """scalars: (n,4) uint64 canonical (`into_repr`). Returns the affine result (Montgomery limbs,
        infinity = zeros). Like arkworks, zips to the shorter of bases/scalars."""
        sc = _u64(scalars)
        out = np.zeros(affine_limbs(bases.curve, bases.group), dtype=np.uint64)
        _chk(LIB.mg_msm(bases.handle, _p(sc), sc.shape[0], _p(out)), "mg_msm")
        return out

    @staticmethod
    def launch(bases: Bases, d_scalars, n, scalars_mont=False, window_bits=0, sparse=False) -> MsmJob:
        """Scalars already in HBM (DeviceBuffer or raw pointer); returns a job to `finish()`."""
        ptr = d_scalars.ptr if isinstance(d_scalars, DeviceBuffer) else d_scalars
        h = _vp()
        _chk(LIB.mg_msm_launch(bases.handle, ptr, n, bool(scalars_mont) | (2 if sparse else 0), window_bits, ctypes.byref(h)),
             "mg_msm_launch")
        return MsmJob(bases, h)

    @staticmethod
    def launch_sharded(bases: Bases, d_scalars_per_shard, scalars_mont=False, window_bits=0, sparse=False) -> MsmJob:
        """Sharded bases, scalars already resident: one DeviceBuffer / pointer per shard, on that shard's device."""
        ptrs = [d.ptr if isinstance(d, DeviceBuffer) else d for d in d_scalars_per_shard]
        arr = (_vp * len(ptrs))(*ptrs)
        h = _vp()
        _chk(LIB.mg_msm_launch_sharded(bases.handle, arr, bool(scalars_mont) | (2 if sparse else 0), window_bits, ctypes.byref(h)),
             "mg_msm_launch_sharded")
        return MsmJob(bases, h)


def blake3(data: bytes) -> bytes:
    """`blake3::hash` (manta-parameters' checksum, lib.rs:173-177), computed by the library's host code"""
    out = ctypes.create_string_buffer(32)
    _chk(LIB.mg_blake3(bytes(data), len(data), out), "mg_blake3")
    return out.raw


def blake2s(data: bytes, digest_size=None) -> bytes:
    """Blake2s-256 (RFC 7693, unkeyed), computed by the library's host code from the source the signature kernels compile; with
    digest_size (1..32) the same hash with a digest of that length (`mg_blake2s`), which is no prefix of the 32-byte one"""
    if digest_size is None:
        out = ctypes.create_string_buffer(32)
        _chk(LIB.mg_blake2s256(bytes(data), len(data), out), "mg_blake2s256")
        return out.raw
    out = ctypes.create_string_buffer(32)
    _chk(LIB.mg_blake2s(bytes(data), len(data), digest_size, out), "mg_blake2s")
    return out.raw[:int(digest_size)]


def aes256_gcm_encrypt(key: bytes, nonce: bytes, plaintext: bytes) -> bytes:
    """AES-256-GCM, 12-byte nonce, no associated data -> ciphertext | 16-byte tag; the library's host code, compiled from the
    source the note kernels compile (`mg_aes256_gcm`)"""
    key, nonce, plaintext = bytes(key), bytes(nonce), bytes(plaintext)
    if len(key) != 32 or len(nonce) != 12:
        raise ValueError("aes256_gcm: a 32-byte key and a 12-byte nonce")
    out = ctypes.create_string_buffer(len(plaintext) + 16)
    _chk(LIB.mg_aes256_gcm(key, nonce, plaintext, len(plaintext), 0, out, None), "mg_aes256_gcm")
    return out.raw


def aes256_gcm_decrypt(key: bytes, nonce: bytes, sealed: bytes):
    """ciphertext | tag -> (plaintext, ok); the plaintext is zeros where the tag does not verify (`mg_aes256_gcm`)"""
    key, nonce, sealed = bytes(key), bytes(nonce), bytes(sealed)
    if len(key) != 32 or len(nonce) != 12 or len(sealed) < 16:
        raise ValueError("aes256_gcm: a 32-byte key, a 12-byte nonce and at least the 16 bytes of a tag")
    out = ctypes.create_string_buffer(max(1, len(sealed) - 16))
    ok = ctypes.c_int(0)
    _chk(LIB.mg_aes256_gcm(key, nonce, sealed, len(sealed), 1, out, ctypes.byref(ok)), "mg_aes256_gcm")
    return out.raw[:len(sealed) - 16], bool(ok.value)


def xyzz_limbs(curve, group) -> int:
    return int(LIB.mg_xyzz_limbs(curve, group))


def xyzz_sum(curve, group, xyzz) -> np.ndarray:
    """sum of XYZZ points (arkworks Montgomery limbs X | Y | ZZ | ZZZ, ZZ = 0: infinity) -> one affine point"""
    pts = _u64(xyzz).reshape(-1, xyzz_limbs(curve, group))
    out = np.zeros(affine_limbs(curve, group), dtype=np.uint64)
    _chk(LIB.mg_xyzz_sum(curve, group, _p(pts), pts.shape[0], _p(out)), "mg_xyzz_sum")
    return out


def points_sum(curve, group, points):
    pts = _u64(points)
    out = np.zeros(affine_limbs(curve, group), dtype=np.uint64)
    _chk(LIB.mg_points_sum(curve, group, _p(pts), pts.shape[0], _p(out)), "mg_points_sum")
    return out


def fixed_base_mul(curve, group, base, d_scalars: DeviceBuffer, n) -> DeviceBuffer:
    out = DeviceBuffer(n * affine_limbs(curve, group) * 8)
    _chk(LIB.mg_fixed_base_mul(curve, group, _p(_u64(base)), d_scalars.ptr, n, out.ptr), "mg_fixed_base_mul")
    return out


EC_ADD_MIXED, EC_ADD, EC_DOUBLE, EC_MUL, EC_SUB_MIXED, EC_MUL_FIXED = range(6)


def group_ntt(curve, group, points, inverse=False) -> np.ndarray:
    """`Radix2EvaluationDomain::{fft, ifft}` over a vector of 2^k group elements (`mg_group_ntt`)."""
    pts = _u64(points)
    n = pts.shape[0]
    lg = n.bit_length() - 1
    assert 1 << lg == n and pts.shape[1] == affine_limbs(curve, group)
    out = np.zeros_like(pts)
    _chk(LIB.mg_group_ntt(curve, group, _p(pts), lg, bool(inverse), _p(out)), "mg_group_ntt")
    return out


def ec_elementwise(curve, group, op, a, b=None) -> np.ndarray:
    """Element-wise group operation on arrays of affine points (`mg_ec_elementwise`; the ecc.rs primitive menu):
    a, b = [n, limbs] uint64 affine points (b = [n, 4] canonical scalars for EC_MUL, unused for EC_DOUBLE)."""
    a = _u64(a)
    n = a.shape[0]
    out = np.zeros_like(a)
    bb = _p(_u64(b)) if b is not None else None
    _chk(LIB.mg_ec_elementwise(curve, group, op, _p(a), bb, n, _p(out)), "mg_ec_elementwise")
    return out


FIELD_IDS = {"bn254_fr": 0, "bn254_fq": 1, "bls381_fr": 2, "bls381_fq": 3}
FIELD_OPS = {"add": 0, "sub": 1, "mul": 2, "sqr": 3, "neg": 4, "from_canonical": 5, "to_canonical": 6, "inv": 7}


def field_op(field, op, a, b=None, repr=0, lazy_a=0, lazy_b=0) -> np.ndarray:
    """Element-wise field arithmetic on the GPU (`mg_field_op`): a, b = [n, limbs] uint64 Montgomery elements of
    `field` ("bn254_fr" ...); repr 0 = the saturated Montgomery arithmetic, 1 = the MSM kernels' reduced-radix lazy
    arithmetic on the representatives a + lazy_a p, b + lazy_b p."""
    a = _u64(a)
    nl = 6 if field == "bls381_fq" else 4
    assert a.ndim == 2 and a.shape[1] == nl, a.shape
    out = np.zeros_like(a)
    bb = None if b is None else _u64(b)
    assert bb is None or bb.shape == a.shape
    _chk(LIB.mg_field_op(FIELD_IDS[field], FIELD_OPS[op], repr, lazy_a, lazy_b, _p(a), _p(bb), a.shape[0], _p(out)), "mg_field_op")
    return out


FPR_OPS = {"mul": 0, "sqr": 1, "mul_add": 2, "sub2_6": 3, "sub2_12": 4}
FPR_LIMBS = {"bn254_fr": (9, 29), "bn254_fq": (9, 29), "bls381_fr": (9, 29), "bls381_fq": (13, 30)}  # (K, LB)


def fpr_raw_op(field, op, a, b=None, c=None, d=None, chain=False) -> np.ndarray:
    """One reduced-radix routine of the MSM kernels over RAW limb vectors (`mg_fpr_raw_op`): a, b, c, d = [n, K] uint32
    limbs, no conversion on the way in or out. op = "mul" | "sqr" | "mul_add" | "sub2_6" | "sub2_12" (a + 6p / 12p - b - 2c).
    chain selects what the accumulate kernel calls: mul_t / sqr_t / mul_add_t<true> and sub2n. For every field those are the
    single-chain codings of the products: asm links for the 29-bit fields, the plain routines' column walker with pinned
    multiply-adds for BLS12-381 Fq (the plain routines themselves with -DMG_CHAIN_FLUSHED=0)."""
    K = FPR_LIMBS[field][0]
    arrs = [None if x is None else np.ascontiguousarray(x, dtype=np.uint32) for x in (a, b, c, d)]
    need = {"sqr": 1, "mul": 2, "sub2_6": 3, "sub2_12": 3, "mul_add": 4}[op]
    for x in arrs[:need]:
        assert x is not None and x.ndim == 2 and x.shape == arrs[0].shape and x.shape[1] == K, (op, None if x is None else x.shape)
    out = np.zeros_like(arrs[0])
    _chk(LIB.mg_fpr_raw_op(FIELD_IDS[field], FPR_OPS[op], bool(chain), _p(arrs[0]), _p(arrs[1]), _p(arrs[2]), _p(arrs[3]),
                           arrs[0].shape[0], _p(out)), "mg_fpr_raw_op")
    return out


PAIRING_OPS = {"mul12": 0, "sqr12": 1, "cyc_sqr12": 2, "ell": 3, "frob12_1": 4, "frob12_2": 5, "frob12_3": 6, "conj12": 7, "inv12": 8,
               "exp_by_x": 9, "final_exp": 10, "fq_inv_euclid": 11, "fq_half": 12, "fq2_mul": 13, "fq2_mul_xi": 14, "fq_lincomb": 15}
PAIRING_LINCOMB_OPERANDS = 10


def pairing_op(curve, op, a, b=None, coeffs=None) -> np.ndarray:
    """One building block of the pairing over n elements (`mg_pairing_op`): uint32 Montgomery words in and out, N = 8 / 12 per
    Fq. Fq12 operations (a = [n, 12 N], arkworks memory order): "mul12" (b = [n, 12 N]), "sqr12", "cyc_sqr12", "ell" (b = [n, 6 N],
    the line's three Fq2 coefficients), "frob12_1" .. "frob12_3", "conj12", "inv12", "exp_by_x", "final_exp". Fq / Fq2 helpers:
    "fq_inv_euclid", "fq_half" (a = [n, N]), "fq2_mul" (a, b = [n, 2 N]), "fq2_mul_xi" (a = [n, 2 N]), "fq_lincomb" (a = [n, 10, N],
    coeffs = [n, 10] integers in -255..255 whose positive and negative sums stay below 256 -> [n, N])."""
    N = 2 * FQ_LIMBS[curve]
    a = np.ascontiguousarray(a, dtype=np.uint32)
    n = a.shape[0]
    if op == "fq_lincomb":
        assert a.shape == (n, PAIRING_LINCOMB_OPERANDS, N), a.shape
        coeffs = np.ascontiguousarray(coeffs, dtype=np.int16)
        assert coeffs.shape == (n, PAIRING_LINCOMB_OPERANDS), coeffs.shape
        out = np.zeros((n, N), dtype=np.uint32)
    else:
        wa = {"fq_inv_euclid": N, "fq_half": N, "fq2_mul": 2 * N, "fq2_mul_xi": 2 * N}.get(op, 12 * N)
        assert a.shape == (n, wa), (op, a.shape)
        coeffs = None
        out = np.zeros_like(a)
    wb = {"mul12": 12 * N, "ell": 6 * N, "fq2_mul": 2 * N}.get(op)
    if wb is not None:
        b = np.ascontiguousarray(b, dtype=np.uint32)
        assert b.shape == (n, wb), (op, b.shape)
    else:
        b = None
    _chk(LIB.mg_pairing_op(curve, PAIRING_OPS[op], _p(a), _p(b), _p(coeffs), n, _p(out)), "mg_pairing_op")
    return out


def fpr_column_plan(field, kind) -> dict:
    """Where the reduced-radix products of `field` flush a column accumulator (`mg_fpr_column_plan`; no GPU needed):
    kind = "mul" | "sqr" | "mul_add" -> dict(flush=[per column: bit 0 / 1 / 2 = before the a b / c d / m p group], peak=[per
    column: worst-case accumulator value], limb_bits, flushed_routines)."""
    flush, peak = np.zeros(25, dtype=np.uint32), np.zeros(25, dtype=np.uint64)
    cols, lb, fr = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
    _chk(LIB.mg_fpr_column_plan(FIELD_IDS[field], FPR_OPS[kind], _p(flush), _p(peak), ctypes.byref(cols), ctypes.byref(lb),
                                ctypes.byref(fr)), "mg_fpr_column_plan")
    return dict(flush=[int(x) for x in flush[:cols.value]], peak=[int(x) for x in peak[:cols.value]], limb_bits=lb.value,
                flushed_routines=bool(fr.value))


def _u32_buffer(a, n, name):
    """the caller's [n] uint32 buffer as a fresh contiguous copy (the library works in place on it), or zeros"""
    out = np.zeros(n, dtype=np.uint32) if a is None else np.array(a, dtype=np.uint32).reshape(-1)
    assert out.shape == (n,), "%s: %d elements, expected %d" % (name, out.size, n)
    return out


def msm_digits(curve, scalars, c, n, mont=False, table_mode=0, map=None, n_sets=1, set_len=None, compact=False, keys=None, vals=None):
    """The MSM's digit kernel alone (`mg_msm_digits`): scalars = [batch, n_scalars, 4] (or [n_scalars, 4]) uint64 against a
    described set of n stored bases -> dict(W, B, seg_keys, invalid, keys, vals, count). keys / vals (batch * W * n uint32,
    default zeros) are what the device arrays hold before the launch; count is None in the fixed layout."""
    sc = _u64(scalars)
    if sc.ndim == 2:
        sc = sc[None]
    assert sc.ndim == 3 and sc.shape[2] == 4, sc.shape
    batch, n_scalars = sc.shape[0], sc.shape[1]
    bits = 254 if curve == BN254 else 255
    W = (bits + c - 1) // c if c > 0 else 0
    size = batch * W * n
    k, v = _u32_buffer(keys, size, "keys"), _u32_buffer(vals, size, "vals")
    mp = None if map is None else np.ascontiguousarray(map, dtype=np.uint32)
    assert mp is None or mp.shape == (n,), mp.shape
    count = ctypes.c_uint32(0)
    layout = (ctypes.c_uint32 * 4)()
    _chk(LIB.mg_msm_digits(curve, _p(sc), batch, n_scalars, bool(mont), c, table_mode, n, _p(mp), n_sets,
                           n if set_len is None else set_len, bool(compact), _p(k), _p(v), ctypes.byref(count) if compact else None,
                           layout), "mg_msm_digits")
    assert layout[0] == W
    return dict(W=int(layout[0]), B=int(layout[1]), seg_keys=int(layout[2]), invalid=int(layout[3]), keys=k, vals=v,
                count=int(count.value) if compact else None)


def msm_dense_front_applies(batch, n_sets, windows, table_mode, sparse):
    """Whether a launch of this shape takes the fused front end (`mg_msm_dense_front_applies`; no device involved)"""
    return bool(LIB.mg_msm_dense_front_applies(batch, n_sets, windows, table_mode, bool(sparse)))


def msm_dense_front(curve, scalars, c, n, mont=False, map=None, set_len=None, keys=None, vals=None):
    """The fused front end alone (`mg_msm_dense_front`): scalars = [n_scalars, 4] uint64 against n stored bases with a table per
    window -> dict(W, B, seg_keys, inf_index, keys, vals): the W * n pairs of all digits, sorted by key; a zero digit is
    (0, inf_index). keys / vals: what the device arrays hold before the launch (default zeros)."""
    sc = _u64(scalars)
    assert sc.ndim == 2 and sc.shape[1] == 4, sc.shape
    bits = 254 if curve == BN254 else 255
    W = (bits + c - 1) // c if c > 0 else 0
    k, v = _u32_buffer(keys, W * n, "keys"), _u32_buffer(vals, W * n, "vals")
    mp = None if map is None else np.ascontiguousarray(map, dtype=np.uint32)
    assert mp is None or mp.shape == (n,), mp.shape
    layout = (ctypes.c_uint32 * 4)()
    _chk(LIB.mg_msm_dense_front(curve, _p(sc), sc.shape[0], bool(mont), c, n, _p(mp), n if set_len is None else set_len, _p(k), _p(v),
                                layout), "mg_msm_dense_front")
    return dict(W=int(layout[0]), B=int(layout[1]), seg_keys=int(layout[2]), inf_index=int(layout[3]), keys=k, vals=v)


def sort_pairs(keys, vals, end_bit, count=None, lowmask=0xFFFFFFFF, inv_from=0xFFFFFFFF, keys_out=None, vals_out=None):
    """The MSM's radix sort alone (`mg_sort_pairs`): [n] uint32 keys below 2^end_bit and their values -> (keys, vals) sorted stably
    by key (by `key >= inv_from ? lowmask + 1 : key & lowmask` when masked). count: only that many pairs exist, read on the device.
    keys_out / vals_out: what the output arrays hold before the launch (default zeros)."""
    k = np.ascontiguousarray(keys, dtype=np.uint32).reshape(-1)
    v = np.ascontiguousarray(vals, dtype=np.uint32).reshape(-1)
    n = k.shape[0]
    assert v.shape == (n,)
    ko, vo = _u32_buffer(keys_out, n, "keys_out"), _u32_buffer(vals_out, n, "vals_out")
    cnt = None if count is None else ctypes.byref(ctypes.c_uint32(count))
    _chk(LIB.mg_sort_pairs(_p(k), _p(v), n, end_bit, cnt, lowmask, inv_from, _p(ko), _p(vo)), "mg_sort_pairs")
    return ko, vo


def point_serialize(curve, group, point, compressed=True):
    nb = FQ_LIMBS[curve] * 8 * (2 if group == 2 else 1) * (1 if compressed else 2)
    out = ctypes.create_string_buffer(nb)
    _chk(LIB.mg_point_serialize(curve, group, _p(_u64(point)), bool(compressed), out), "mg_point_serialize")
    return out.raw


class Radix2EvaluationDomain:
    """Mirror of ark_poly::Radix2EvaluationDomain<Fr> (ark-poly 0.3.0)."""

    def __init__(self, curve, size):
        self.curve = curve
        self.log_size = max(0, (int(size) - 1).bit_length())
        self.size = 1 << self.log_size

    def _run(self, data, inverse, coset):
        d = np.array(data, dtype=np.uint64, copy=True)
        assert d.shape == (self.size, 4)
        _chk(LIB.mg_ntt(self.curve, _p(d), self.log_size, inverse, coset), "mg_ntt")
        return d

    def fft(self, data):
        return self._run(data, False, False)

    def ifft(self, data):
        return self._run(data, True, False)

    def coset_fft(self, data):
        return self._run(data, False, True)

    def coset_ifft(self, data):
        return self._run(data, True, True)

    def fft_device(self, dbuf: DeviceBuffer, inverse=False, coset=False):
        _chk(LIB.mg_ntt_device(self.curve, dbuf.ptr, self.log_size, bool(inverse), bool(coset)), "mg_ntt_device")


# ------------------------------------------------------------------------------------------------ Groth16
class _PkView(ctypes.Structure):
    _fields_ = [("n_vars", ctypes.c_uint64), ("n_inputs", ctypes.c_uint64), ("h_len", ctypes.c_uint64)] + [
        (k, _vp) for k in ("alpha_g1", "beta_g1", "delta_g1", "beta_g2", "delta_g2", "a_query", "b_g1_query",
                           "b_g2_query", "h_query", "l_query")]


class _Csr(ctypes.Structure):
    _fields_ = [("row_ptr", _vp), ("col", _vp), ("val", _vp), ("nnz", ctypes.c_uint64)]


class R1CS:
    """Mirror of manta_crypto::arkworks::constraint::R1CS<F> as the prover sees it: the matrices of
    `cs.to_matrices()` and the full assignment z = instance || witness (Montgomery Fr)."""

    def __init__(self, curve, A, B, C, num_constraints, num_instance, z):
        self.curve, self.A, self.B, self.C = curve, A, B, C
        self.num_constraints, self.num_instance = int(num_constraints), int(num_instance)
        self.z = _u64(z)

    @classmethod
    def from_circuit(cls, c):
        return cls(c.curve, c.A, c.B, c.C, c.m, c.P, c.z)

    def which_is_unsatisfied(self):
        """The lowest constraint row the compiler's own assignment fails, or None (ark-relations `which_is_unsatisfied`,
        which names the row; checked on the GPU by `mg_r1cs_check`, no proving key needed)."""
        first, _ = r1cs_check(self.curve, self.A, self.B, self.C, self.num_constraints, self.z.size // 4, self.z)
        return None if first[0] < 0 else int(first[0])

    def is_satisfied(self) -> bool:
        """`R1CS::is_satisfied` (manta-crypto/src/arkworks/constraint/mod.rs:130-132)."""
        return self.which_is_unsatisfied() is None


class _PkOut(ctypes.Structure):
    _fields_ = [(n, _vp) for n in ("alpha_g1", "beta_g1", "delta_g1", "beta_g2", "gamma_g2", "delta_g2", "gamma_abc_g1",
                                   "a_query", "b_g1_query", "b_g2_query", "h_query", "l_query")]


class ProvingKey:
    """Host arrays in the C ABI's memory format (affine Montgomery limbs, infinity = zeros): the fields of
    ark_groth16::ProvingKey (incl. its verifying key) that `ProvingContext` and a verifier consume."""
    pass


def groth16_setup(r1cs: "R1CS", n_vars, toxic_mont, g1_generator, g2_generator) -> ProvingKey:
    """Mirror of `Groth16::compile` (manta-crypto/src/arkworks/groth16.rs:571-586) with the randomness made explicit
    (`mg_groth16_setup`): toxic_mont = alpha, beta, gamma, delta, tau as Montgomery Fr (5 x 4 u64), the generators as
    affine points. Every group element of the key is computed on the GPU."""
    curve, m, P, V = r1cs.curve, r1cs.num_constraints, r1cs.num_instance, int(n_vars)
    D = 1
    while D < m + P:
        D <<= 1
    w1, w2 = affine_limbs(curve, 1), affine_limbs(curve, 2)
    pk = ProvingKey()
    pk.curve, pk.V, pk.P, pk.D, pk.h_len = curve, V, P, D, D - 1
    shapes = {"alpha_g1": (1, w1), "beta_g1": (1, w1), "delta_g1": (1, w1), "beta_g2": (1, w2), "gamma_g2": (1, w2),
              "delta_g2": (1, w2), "gamma_abc_g1": (P, w1), "a_query": (V, w1), "b_g1_query": (V, w1),
              "b_g2_query": (V, w2), "h_query": (D - 1, w1), "l_query": (V - P, w1)}
    for k, sh in shapes.items():
        setattr(pk, k, np.zeros(sh, dtype=np.uint64))
    out = _PkOut(*[_p(getattr(pk, k)) for k, _ in _PkOut._fields_])
    ms = []
    for M in (r1cs.A, r1cs.B, r1cs.C):
        rp = np.ascontiguousarray(M.row_ptr, dtype=np.uint32)
        col = np.ascontiguousarray(M.col, dtype=np.uint32)
        val = _u64(M.val)
        ms.append((rp, col, val, _Csr(_p(rp), _p(col), _p(val), len(col))))
    tox = _u64(toxic_mont).reshape(5, 4)
    _chk(LIB.mg_groth16_setup(curve, ctypes.byref(ms[0][3]), ctypes.byref(ms[1][3]), ctypes.byref(ms[2][3]), m, V, P, _p(tox),
                              _p(_u64(g1_generator)), _p(_u64(g2_generator)), ctypes.byref(out)), "mg_groth16_setup")
    return pk


def _csr(M):
    """a matrix with row_ptr / col / val arrays -> (the arrays kept alive, the mg_csr over them)"""
    rp = np.ascontiguousarray(M.row_ptr, dtype=np.uint32)
    col = np.ascontiguousarray(M.col, dtype=np.uint32)
    val = _u64(M.val)
    return (rp, col, val), _Csr(_p(rp), _p(col), _p(val), len(col))


R1CS_SATISFIED = (1 << 64) - 1  # MG_R1CS_SATISFIED


def _r1cs_verdicts(first, count):
    """the C ABI's u64 outputs -> (first, counts) as int64 arrays, -1 for a satisfied assignment"""
    return np.where(first == np.uint64(R1CS_SATISFIED), np.int64(-1), first.astype(np.int64)), count.astype(np.int64)


def r1cs_check(curve, A, B, C, m, n_vars, zs):
    """`mg_r1cs_check`: which of the assignments zs (k x n_vars x 4 u64 Montgomery) satisfy the m constraint rows of A, B, C
    (matrices with row_ptr / col / val). Returns (first, counts): per assignment the lowest failing row (-1: satisfied) and
    the number of failing rows."""
    zs = _u64(zs)
    n_vars = int(n_vars)
    if n_vars > 0 and zs.size % (n_vars * 4):
        raise ValueError(f"assignments hold {zs.size} u64 words, no multiple of n_vars x 4 = {n_vars * 4}")
    k = zs.size // (n_vars * 4) if n_vars > 0 else 0
    keep = [_csr(M) for M in (A, B, C)]
    first, count = np.zeros(k, dtype=np.uint64), np.zeros(k, dtype=np.uint64)
    _chk(LIB.mg_r1cs_check(curve, ctypes.byref(keep[0][1]), ctypes.byref(keep[1][1]), ctypes.byref(keep[2][1]), m, n_vars, k, _p(zs),
                           _p(first), _p(count)), "mg_r1cs_check")
    return _r1cs_verdicts(first, count)


def qap_columns(curve, group, bases, mats, n_cols, entries_per_lane=0) -> np.ndarray:
    """Column sums of scaled group elements (`mg_qap_columns`; `specialize_to_phase_2`, mpc.rs:251-294):
    out[j] = sum over t and the stored entries (i, j) of mats[t] of [mats[t][i][j]] bases[t][i]. bases: a list of [m, limbs]
    uint64 affine point arrays, mats: as many CSR matrices (row_ptr[m + 1], col, val Montgomery Fr) of m rows and n_cols
    columns. Returns [n_cols, limbs] affine points. entries_per_lane places the chunk boundaries of the segmented sum (0: the
    library's choice); no result depends on it."""
    bases = [_u64(b) for b in bases]
    if len(bases) != len(mats):
        raise ValueError("qap_columns: one basis per matrix")
    m = len(mats[0].row_ptr) - 1 if mats else 0
    for b, M in zip(bases, mats):
        if b.ndim != 2 or b.shape != (m, affine_limbs(curve, group)) or len(M.row_ptr) != m + 1:
            raise ValueError("qap_columns: every basis is [m, limbs] and every matrix has m rows")
    keep = [_csr(M) for M in mats]
    bp = (ctypes.c_void_p * max(len(bases), 1))(*[b.ctypes.data for b in bases])
    mp = (ctypes.POINTER(_Csr) * max(len(mats), 1))(*[ctypes.pointer(k[1]) for k in keep])
    out = np.zeros((int(n_cols), affine_limbs(curve, group)), dtype=np.uint64)
    _chk(LIB.mg_qap_columns(curve, group, len(bases), bp, mp, m, n_cols, entries_per_lane, _p(out)), "mg_qap_columns")
    return out


class _KzgView(ctypes.Structure):
    _fields_ = [("n_g1", ctypes.c_uint64), ("n_g2", ctypes.c_uint64)] + [
        (k, _vp) for k in ("tau_powers_g1", "tau_powers_g2", "alpha_tau_powers_g1", "beta_tau_powers_g1", "beta_g2")]


def mpc_initialize(curve, tau_powers_g1, tau_powers_g2, alpha_tau_powers_g1, beta_tau_powers_g1, beta_g2, r1cs: "R1CS", n_vars,
                   h_len, g1_generator, g2_generator) -> ProvingKey:
    """`mpc::initialize` (manta-trusted-setup/src/groth16/mpc.rs:353-431; `mg_mpc_initialize`): the phase-2 proving key of a
    circuit from the vectors of a KZG accumulator, gamma = delta = 1 (the generators passed in). h_len = D - 1 (the length
    ark-groth16 keys carry) or D (the reference's loop). The Lagrange bases and the QAP column sums are computed on the GPU;
    only the key comes back."""
    m, P, V = r1cs.num_constraints, r1cs.num_instance, int(n_vars)
    D = 1
    while D < m + P:
        D <<= 1
    h_len = int(h_len)
    w1, w2 = affine_limbs(curve, 1), affine_limbs(curve, 2)
    vecs = [_u64(v) for v in (tau_powers_g1, tau_powers_g2, alpha_tau_powers_g1, beta_tau_powers_g1, beta_g2)]
    view = _KzgView(vecs[0].shape[0], min(v.shape[0] for v in vecs[1:4]), *[_p(v) for v in vecs])
    pk = ProvingKey()
    pk.curve, pk.V, pk.P, pk.D, pk.h_len = curve, V, P, D, h_len
    shapes = {"alpha_g1": (1, w1), "beta_g1": (1, w1), "delta_g1": (1, w1), "beta_g2": (1, w2), "gamma_g2": (1, w2),
              "delta_g2": (1, w2), "gamma_abc_g1": (P, w1), "a_query": (V, w1), "b_g1_query": (V, w1),
              "b_g2_query": (V, w2), "h_query": (max(h_len, 0), w1), "l_query": (max(V - P, 0), w1)}
    for k, sh in shapes.items():
        setattr(pk, k, np.zeros(sh, dtype=np.uint64))
    out = _PkOut(*[_p(getattr(pk, k)) for k, _ in _PkOut._fields_])
    keep = [_csr(M) for M in (r1cs.A, r1cs.B, r1cs.C)]
    _chk(LIB.mg_mpc_initialize(curve, ctypes.byref(view), ctypes.byref(keep[0][1]), ctypes.byref(keep[1][1]),
                               ctypes.byref(keep[2][1]), m, V, P, h_len, _p(_u64(g1_generator)), _p(_u64(g2_generator)),
                               ctypes.byref(out)), "mg_mpc_initialize")
    return pk


EXCHANGE_HOST, EXCHANGE_RCCL = 0, 1


class Tuning(ctypes.Structure):
    """`mg_tuning` (include/mantagpu.h): what a deployment decides about the library's scheduling -- process-wide through
    get_tuning / set_tuning, per context through ProvingContext(tuning=...). No field changes a result."""
    _fields_ = [("struct_size", ctypes.c_uint32), ("graph_mode", ctypes.c_int32), ("graph_mode_batch", ctypes.c_int32),
                ("prove_streams", ctypes.c_int32), ("linear_chains", ctypes.c_int32), ("coalesce_inflight", ctypes.c_int32),
                ("coalesce_gather_us", ctypes.c_int32), ("batch_inflight", ctypes.c_int32), ("queue_aware", ctypes.c_int32),
                ("msm_dedicated_queues", ctypes.c_int32), ("window_bits_narrow", ctypes.c_int32), ("window_bits_wide", ctypes.c_int32),
                ("window_bits_h", ctypes.c_int32), ("window_bits_g2", ctypes.c_int32), ("full_table_bytes", ctypes.c_int64)]

    def replace(self, **kw):
        t = Tuning.from_buffer_copy(bytes(self))
        for k, v in kw.items():
            if k not in dict(Tuning._fields_) or k == "struct_size":
                raise ValueError("mg_tuning has no field %r" % k)
            setattr(t, k, int(v))
        return t

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in Tuning._fields_ if k != "struct_size"}


GRAPH_OFF, GRAPH_SINGLE, GRAPH_SPLIT = 0, 1, 2


def tuning_defaults() -> Tuning:
    t = Tuning()
    _chk(LIB.mg_tuning_init(ctypes.byref(t)), "mg_tuning_init")
    assert t.struct_size == ctypes.sizeof(Tuning), "mg_tuning: the Python mirror is out of date"
    return t


def get_tuning() -> Tuning:
    t = Tuning()
    _chk(LIB.mg_get_tuning(ctypes.byref(t)), "mg_get_tuning")
    return t


def set_tuning(t: Tuning = None, **kw):
    """process-wide tuning for contexts created from now on: a whole struct, or keyword changes to the values in force"""
    t = (t if t is not None else get_tuning()).replace(**kw)
    _chk(LIB.mg_set_tuning(ctypes.byref(t)), "mg_set_tuning")


def tuning_env_names() -> list:
    """the environment variables the shipped library reads (mg_tuning_env_names)"""
    arr, out, i = LIB.mg_tuning_env_names(), [], 0
    while arr[i]:
        out.append(arr[i].decode())
        i += 1
    return out


class _CtxOpts(ctypes.Structure):
    """`mg_ctx_opts` (include/mantagpu.h)"""
    _fields_ = [("struct_size", ctypes.c_uint32), ("exchange", ctypes.c_uint32), ("full_table_bytes", ctypes.c_int64),
                ("devices", ctypes.POINTER(ctypes.c_int)), ("n_devices", ctypes.c_int32), ("shard", ctypes.c_int32),
                ("n_shards", ctypes.c_int32), ("task_mask", ctypes.c_uint32), ("tuning", ctypes.POINTER(Tuning))]


def _ctx_opts(devices=None, shard=None, task_mask=None, full_table_bytes=None, exchange=None, tuning=None):
    """-> (mg_ctx_opts, keep-alive) from the keyword arguments of ProvingContext"""
    o = _CtxOpts()
    _chk(LIB.mg_ctx_opts_init(ctypes.byref(o)), "mg_ctx_opts_init")
    assert o.struct_size == ctypes.sizeof(_CtxOpts), "mg_ctx_opts: the Python mirror is out of date"
    keep = None
    if devices is not None:
        keep = (ctypes.c_int * len(devices))(*devices)
        o.devices, o.n_devices = keep, len(devices)
    if shard is not None:
        o.shard, o.n_shards = int(shard[0]), int(shard[1])
    if task_mask is not None:
        o.task_mask = int(task_mask)
    if full_table_bytes is not None:
        o.full_table_bytes = int(full_table_bytes)
    if exchange is not None:
        o.exchange = int(exchange)
    if tuning is not None:
        if isinstance(tuning, dict):
            tuning = get_tuning().replace(**tuning)
        o.tuning = ctypes.pointer(tuning)
        keep = (keep, tuning)
    return o, keep


class ProvingContext:
    """Mirror of groth16::ProvingContext<E> (manta-crypto/src/arkworks/groth16.rs:216-245): owns the
    device-resident proving key; created once, shared by every proof of the shape."""

    def __init__(self, curve, pk, devices=None, shard=None, task_mask=None, full_table_bytes=None, exchange=None, tuning=None):
        """pk: object with numpy arrays alpha_g1, beta_g1, delta_g1, beta_g2, delta_g2, a_query,
        b_g1_query, b_g2_query, h_query, l_query (affine Montgomery limbs) and ints V, P.
        devices: list of HIP device indices -> every MSM of a proof is range-sharded over them
        (`mg_ctx_create_sharded`); None -> the current device.
        shard = (g, G): this PROCESS holds slice g of G of every query on the current device (`mg_ctx_create_shard`,
        one process per GPU; see distributed.ShardedProver).
        full_table_bytes: HBM budget of the context's full tables (None = the library's default, a tenth of the device's
        HBM; 0 = bucket tables only); exchange: EXCHANGE_HOST / EXCHANGE_RCCL for a `devices` list (`mg_ctx_opts`);
        tuning: this context's `Tuning` (or a dict of field changes to the process-wide values), `mg_ctx_opts.tuning`."""
        self.curve = curve
        self._keep = [_u64(getattr(pk, k)) for k in ("alpha_g1", "beta_g1", "delta_g1", "beta_g2", "delta_g2",
                                                     "a_query", "b_g1_query", "b_g2_query", "h_query", "l_query")]
        v = _PkView(pk.V, pk.P, self._keep[8].shape[0], *[_p(a) for a in self._keep])
        h = _vp()
        if task_mask is not None and int(task_mask) == 0:  # a rank beyond the fifth owns no MSM: the struct reads 0 as "all five"
            _chk(LIB.mg_ctx_create_task(curve, ctypes.byref(v), 0, ctypes.byref(h)), "mg_ctx_create_task")
        elif shard is not None and int(shard[1]) == 1 and devices is None and task_mask is None and full_table_bytes is None and tuning is None:
            # a world of one driven through the partials interface: the entry point that says so (no combined a | b_g1 | l table)
            _chk(LIB.mg_ctx_create_shard(curve, ctypes.byref(v), 0, 1, ctypes.byref(h)), "mg_ctx_create_shard")
        else:
            o, keep = _ctx_opts(devices, shard, task_mask, full_table_bytes, exchange, tuning)
            _chk(LIB.mg_ctx_create_ex(curve, ctypes.byref(v), ctypes.byref(o), ctypes.byref(h)), "mg_ctx_create_ex")
            del keep
        self._keep = None  # the library copied everything
        self.handle = h
        self._r1cs_ref = None

    @classmethod
    def decode(cls, curve, data: bytes, devices=None, checksum: bytes = None, full_table_bytes=None, exchange=None, tuning=None):
        """Mirror of `impl Decode for ProvingContext` (groth16.rs:268-288): arkworks `deserialize_unchecked`
        bytes of the ProvingKey -- the format of manta-parameters' proving-key files. checksum: the file's BLAKE3 digest as
        manta-parameters' data.checkfile lists it (32 bytes); a mismatch raises before anything is uploaded, whatever the
        placement (`manta_parameters::verify`, manta-parameters/src/lib.rs:173-177; `mg_ctx_create_from_bytes_ex`)."""
        self = cls.__new__(cls)
        self.curve = curve
        self._keep = None
        self._r1cs_ref = None
        h = _vp()
        if checksum is not None and len(checksum) != 32:
            raise ValueError("a BLAKE3 digest is 32 bytes")
        o, keep = _ctx_opts(devices, None, None, full_table_bytes, exchange, tuning)
        _chk(LIB.mg_ctx_create_from_bytes_ex(curve, bytes(data), len(data), None if checksum is None else bytes(checksum),
                                             ctypes.byref(o), ctypes.byref(h)), "mg_ctx_create_from_bytes_ex")
        del keep
        self.handle = h
        return self

    @property
    def num_variables(self):
        """V: the number of Fr elements every assignment must have (from the C context, so the decode() path knows it too)."""
        return int(LIB.mg_ctx_num_variables(self.handle))

    @property
    def num_inputs(self):
        return int(LIB.mg_ctx_num_inputs(self.handle))

    @property
    def num_shards(self):
        return int(LIB.mg_ctx_num_shards(self.handle))

    def _check_assignment(self, z, k=1):
        """The C side copies k*V*32 bytes from the buffer: a short array must never reach it."""
        z = np.ascontiguousarray(z, dtype=np.uint64)
        want = k * self.num_variables * 4
        if z.size != want:
            raise ValueError(f"assignment holds {z.size} u64 words, the context's circuit needs {want} ({k} x V = {self.num_variables} x 4)")
        return z

    def set_r1cs(self, r1cs: R1CS):
        ms = []
        for M in (r1cs.A, r1cs.B, r1cs.C):
            rp = np.ascontiguousarray(M.row_ptr, dtype=np.uint32)
            col = np.ascontiguousarray(M.col, dtype=np.uint32)
            val = _u64(M.val)
            ms.append((rp, col, val, _Csr(_p(rp), _p(col), _p(val), len(col))))
        _chk(LIB.mg_ctx_set_r1cs(self.handle, ctypes.byref(ms[0][3]), ctypes.byref(ms[1][3]), ctypes.byref(ms[2][3]),
                                 r1cs.num_constraints), "mg_ctx_set_r1cs")
        import weakref
        self._r1cs_ref = weakref.ref(r1cs)  # the uploaded matrices belong to exactly this R1CS object

    @property
    def domain_size(self):
        return LIB.mg_ctx_domain_size(self.handle)

    def table_bytes(self):
        """HBM bytes of the key tables: (bucket tables, full tables)"""
        v = (ctypes.c_uint64 * 2)()
        _chk(LIB.mg_ctx_table_bytes(self.handle, v), "mg_ctx_table_bytes")
        return int(v[0]), int(v[1])

    # ---- process-per-GPU sharding: partial results on the device, gathered by a collective, assembled on the host
    @property
    def partials_slot_limbs(self):
        return int(LIB.mg_partials_slot_limbs(self.handle))

    def partials_launch(self, zs, k, d_out_ptr, stream=None):
        """`mg_groth16_partials_launch`: this shard's five partial MSM results of k proofs -> device memory at d_out_ptr
        ([k][5][slot] u64); `stream` waits for them. Returns a handle for partials_finish()."""
        zs = self._check_assignment(zs, k)
        h = _vp()
        _chk(LIB.mg_groth16_partials_launch(self.handle, k, _p(zs), _addr(d_out_ptr), _addr(stream), ctypes.byref(h)),
             "mg_groth16_partials_launch")
        return h

    @staticmethod
    def partials_finish(job):
        _chk(LIB.mg_groth16_partials_finish(job), "mg_groth16_partials_finish")

    def assemble(self, parts, rs, ss) -> list:
        """`mg_groth16_assemble`: parts [n_parts][k][5][slot] u64 (the gathered partial results), rs / ss k blinding
        scalars each -> k proofs (bytes)."""
        rs = np.ascontiguousarray(rs, dtype=np.uint64).reshape(-1, 4)
        ss = np.ascontiguousarray(ss, dtype=np.uint64).reshape(-1, 4)
        k = rs.shape[0]
        slot = self.partials_slot_limbs
        parts = np.ascontiguousarray(parts, dtype=np.uint64).reshape(-1, k, 5, slot)
        n = PROOF_BYTES[self.curve]
        out = ctypes.create_string_buffer(n * k)
        _chk(LIB.mg_groth16_assemble(self.handle, k, parts.shape[0], _p(parts), _p(rs), _p(ss), out), "mg_groth16_assemble")
        return [out.raw[i * n:(i + 1) * n] for i in range(k)]

    def witness_map(self, z):
        h = np.zeros((self.domain_size, 4), dtype=np.uint64)
        z = self._check_assignment(z)
        _chk(LIB.mg_witness_map(self.handle, _p(z), _p(h)), "mg_witness_map")
        return h

    def check_assignments(self, zs):
        """`mg_ctx_r1cs_check`: zs = any number of assignments of the context's circuit (k x V x 4 u64) against the matrices
        of the last set_r1cs. Returns (first, counts) as int64 arrays: per assignment the lowest unsatisfied constraint row
        (-1: satisfied -- what ark-groth16's debug_assert! in create_proof checks) and the number of unsatisfied rows."""
        zs = np.ascontiguousarray(zs, dtype=np.uint64)
        k = zs.size // (self.num_variables * 4)
        zs = self._check_assignment(zs, k)
        first, count = np.zeros(k, dtype=np.uint64), np.zeros(k, dtype=np.uint64)
        _chk(LIB.mg_ctx_r1cs_check(self.handle, k, _p(zs), _p(first), _p(count)), "mg_ctx_r1cs_check")
        return _r1cs_verdicts(first, count)

    def close(self):
        if self.handle is not None:
            LIB.mg_ctx_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


PROOF_BYTES = {BN254: 128, BLS12_381: 192}


class Groth16:
    """Mirror of `impl ProofSystem for Groth16<E>` (manta-crypto/src/arkworks/groth16.rs:548-610), prove only."""

    @staticmethod
    def prove(context: ProvingContext, compiler: R1CS, rng) -> bytes:
        """`rng` supplies the two blinding scalars exactly where ark-groth16's create_random_proof draws
        them: r = Fr::rand(rng); s = Fr::rand(rng) -- `rng()` must return one Montgomery Fr element
        (4 x u64) per call. Returns the arkworks canonical compressed proof bytes."""
        # the matrices on the device are those of the R1CS object last uploaded: another object -- even one with the
        # same (m, P) -- is another circuit and is uploaded afresh
        if context._r1cs_ref is None or context._r1cs_ref() is not compiler:
            context.set_r1cs(compiler)
        r = _u64(rng())
        s = _u64(rng())
        return Groth16.prove_with_randomness(context, compiler.z, r, s)

    @staticmethod
    def prove_with_randomness(context: ProvingContext, z, r, s) -> bytes:
        out = ctypes.create_string_buffer(PROOF_BYTES[context.curve])
        z = context._check_assignment(z)
        r, s = _u64(r).reshape(-1), _u64(s).reshape(-1)
        if r.size != 4 or s.size != 4:
            raise ValueError("r and s are one Fr element (4 x u64) each")
        _chk(LIB.mg_groth16_prove(context.handle, _p(z), _p(r), _p(s), out), "mg_groth16_prove")
        return out.raw

    @staticmethod
    def prove_batch(context: ProvingContext, zs, rs, ss) -> list:
        """k proofs of the context's circuit in one pass of the GPU pipeline (`mg_groth16_prove_batch`): zs = k
        assignments (k x V x 4 u64), rs / ss = k blinding scalars each. Returns k proofs, proof q byte-identical to
        prove_with_randomness(context, zs[q], rs[q], ss[q])."""
        zs = np.ascontiguousarray(zs, dtype=np.uint64)
        rs = np.ascontiguousarray(rs, dtype=np.uint64).reshape(-1, 4)
        ss = np.ascontiguousarray(ss, dtype=np.uint64).reshape(-1, 4)
        k = rs.shape[0]
        if ss.shape[0] != k or k == 0:
            raise ValueError("prove_batch: zs, rs, ss must describe the same number of proofs")
        zs = context._check_assignment(zs, k)
        n = PROOF_BYTES[context.curve]
        out = ctypes.create_string_buffer(n * k)
        _chk(LIB.mg_groth16_prove_batch(context.handle, k, _p(zs), _p(rs), _p(ss), out), "mg_groth16_prove_batch")
        return [out.raw[i * n:(i + 1) * n] for i in range(k)]


def pairing_check(curve, g1_points, g2_points) -> bool:
    """prod_i e(P_i, Q_i) == 1 (`mg_pairing_check`): the test behind `PairingEngineExt::has_same` / `same_ratio`
    (manta-crypto/src/arkworks/pairing.rs:88-109). g1_points [n, 2 * limbs], g2_points [n, 4 * limbs] affine Montgomery."""
    g1 = _u64(g1_points).reshape(-1, affine_limbs(curve, 1))
    g2 = _u64(g2_points).reshape(-1, affine_limbs(curve, 2))
    if g1.shape[0] != g2.shape[0] or g1.shape[0] == 0:
        raise ValueError("pairing_check: as many G1 as G2 points, at least one")
    ok = ctypes.c_int(0)
    _chk(LIB.mg_pairing_check(curve, _p(g1), _p(g2), g1.shape[0], ctypes.byref(ok)), "mg_pairing_check")
    return bool(ok.value)


def proof_decode(curve, proof_bytes) -> np.ndarray:
    """Mirror of `Proof::deserialize`: arkworks compressed a | b | c -> affine Montgomery limbs (a | b | c), checked."""
    out = np.zeros(2 * affine_limbs(curve, 1) + affine_limbs(curve, 2), dtype=np.uint64)
    _chk(LIB.mg_proof_decode(curve, bytes(proof_bytes), _p(out)), "mg_proof_decode")
    return out


# per-point status of the batched codec (mantagpu.h MG_POINT_*)
POINT_OK, POINT_BAD_ENCODING, POINT_NOT_ON_CURVE, POINT_NOT_IN_SUBGROUP = 0, 1, 2, 3


def point_bytes(curve, group, compressed=True):
    """bytes of one arkworks point encoding: 32 / 48 (G1), 64 / 96 (G2), twice that uncompressed"""
    return FQ_LIMBS[curve] * 8 * (2 if group == 2 else 1) * (1 if compressed else 2)


def _joined(data):
    return bytes(data) if isinstance(data, (bytes, bytearray, memoryview)) else b"".join(bytes(d) for d in data)


def points_decode(curve, group, data, compressed=True, checked=True):
    """Batched `CanonicalDeserialize` of arkworks point encodings on the GPU (`mg_points_decode`): data = the encodings
    back to back (or a sequence of them). Returns (points [n, limbs] affine Montgomery, zeros for infinity and for rejected
    points; status [n] uint8, POINT_*). checked=False is `deserialize_unchecked` (uncompressed only)."""
    data = _joined(data)
    nb = point_bytes(curve, group, compressed)
    if len(data) % nb:
        raise ValueError(f"{len(data)} bytes is not a whole number of {nb}-byte encodings")
    n = len(data) // nb
    out = np.zeros((n, affine_limbs(curve, group)), dtype=np.uint64)
    st = np.zeros(n, dtype=np.uint8)
    _chk(LIB.mg_points_decode(curve, group, data, n, bool(compressed), bool(checked), _p(out), _p(st), None), "mg_points_decode")
    return out, st


def points_check(curve, group, points) -> np.ndarray:
    """`C::check` / `State::check` on the GPU (`mg_points_check`): status [n] uint8 (POINT_*) of affine Montgomery points."""
    pts = _u64(points).reshape(-1, affine_limbs(curve, group))
    st = np.zeros(pts.shape[0], dtype=np.uint8)
    _chk(LIB.mg_points_check(curve, group, _p(pts), pts.shape[0], _p(st), None), "mg_points_check")
    return st


def points_encode(curve, group, points, compressed=True) -> bytes:
    """Batched `CanonicalSerialize` on the GPU (`mg_points_encode`): the encodings back to back, each byte for byte
    `point_serialize`."""
    pts = _u64(points).reshape(-1, affine_limbs(curve, group))
    out = ctypes.create_string_buffer(max(1, pts.shape[0] * point_bytes(curve, group, compressed)))
    _chk(LIB.mg_points_encode(curve, group, _p(pts), pts.shape[0], bool(compressed), out), "mg_points_encode")
    return out.raw[:pts.shape[0] * point_bytes(curve, group, compressed)]


def ppot_point_bytes(group, compressed):
    """bytes of one record of a Perpetual Powers of Tau file (Bn254): 64 / 32 (G1), 128 / 64 (G2)"""
    return point_bytes(BN254, group, compressed)


def _byte_view(data):
    """a uint8 view of any buffer-protocol object (bytes, memoryview, mmap, ...): no copy, read-only buffers included"""
    return np.frombuffer(data, dtype=np.uint8) if len(data) else np.zeros(0, dtype=np.uint8)


def ppot_points_decode(group, data, compressed, checked=True):
    """Batched `PpotSerializer` reads on the GPU (`mg_ppot_points_decode`, Bn254): data = the records back to back, any
    buffer (or a sequence of buffers, joined). Returns (points [n, limbs] affine Montgomery, zeros for infinity and for
    rejected points; status [n] uint8, POINT_*). checked=False is `deserialize_unchecked` / `deserialize_compressed`, which
    leave the curve (uncompressed) and subgroup tests out."""
    if isinstance(data, (list, tuple)):
        data = b"".join(data)
    view = _byte_view(data)
    nb = ppot_point_bytes(group, compressed)
    if view.size % nb:
        raise ValueError(f"{view.size} bytes is not a whole number of {nb}-byte records")
    n = view.size // nb
    out = np.zeros((n, affine_limbs(BN254, group)), dtype=np.uint64)
    st = np.zeros(n, dtype=np.uint8)
    _chk(LIB.mg_ppot_points_decode(BN254, group, _p(view), n, bool(compressed), bool(checked), _p(out), _p(st), None), "mg_ppot_points_decode")
    return out, st


def ppot_points_encode(group, points, compressed) -> bytes:
    """Batched `PpotSerializer` writes on the GPU (`mg_ppot_points_encode`, Bn254): the records back to back."""
    pts = _u64(points).reshape(-1, affine_limbs(BN254, group))
    nb = pts.shape[0] * ppot_point_bytes(group, compressed)
    out = ctypes.create_string_buffer(max(1, nb))
    _chk(LIB.mg_ppot_points_encode(BN254, group, _p(pts), pts.shape[0], bool(compressed), out), "mg_ppot_points_encode")
    return out.raw[:nb]


def blake2b512(data) -> bytes:
    """Blake2b-512 (RFC 7693, unkeyed) of any buffer, read in place by the library's host code (`mg_blake2b512`): the hash of
    PPoT file headers and responses"""
    view = _byte_view(data)
    out = ctypes.create_string_buffer(64)
    _chk(LIB.mg_blake2b512(_p(view), view.size, out), "mg_blake2b512")
    return out.raw


def proofs_decode(curve, proofs):
    """k proofs (byte strings, or their concatenation) decoded and checked on the GPU (`mg_proofs_decode`). Returns
    (points [k, limbs] a | b | c rows as `proof_decode` gives, zeros where rejected; ok [k] bool: proof_decode would
    accept proof i)."""
    data = _joined(proofs)
    pb = 4 * FQ_LIMBS[curve] * 8
    if len(data) % pb:
        raise ValueError(f"{len(data)} bytes is not a whole number of {pb}-byte proofs")
    k = len(data) // pb
    out = np.zeros((k, 2 * affine_limbs(curve, 1) + affine_limbs(curve, 2)), dtype=np.uint64)
    ok = np.zeros(k, dtype=np.uint8)
    _chk(LIB.mg_proofs_decode(curve, data, k, _p(out), _p(ok)), "mg_proofs_decode")
    return out, ok.astype(bool)


POSEIDON_CHUNK = 1 << 19  # MG_POSEIDON_CHUNK: states per device pass of permute / hash
# (full, partial) rounds per width of manta-pay's Poseidon specifications (manta-pay/src/config/poseidon.rs:26-48)
POSEIDON_ROUNDS = {3: (8, 55), 4: (8, 55), 5: (8, 56), 6: (8, 56)}


def poseidon_param_count(width, full_rounds, partial_rounds):
    """field elements of a `Hasher` encoding: round keys, MDS matrix, domain tag"""
    return (full_rounds + partial_rounds) * width + width * width + 1


class PoseidonHasher:
    """`Hasher<S, T, ARITY>` (manta-pay/src/crypto/poseidon/hash.rs) over Fr of `curve`, run on the GPU one state per lane:
    `permute` (the Poseidon permutation), `hash` (word 0 of the permutation of (domain tag, inputs)) and `hash_device`.
    Elements are [.., 4] uint64 Montgomery limbs."""

    def __init__(self, curve, width, full_rounds, partial_rounds, data):
        self._h = _vp()
        self.curve, self.width, self.full_rounds, self.partial_rounds = curve, width, full_rounds, partial_rounds
        data = bytes(data)
        _chk(LIB.mg_poseidon_create(curve, width, full_rounds, partial_rounds, data, len(data),
                                    ctypes.byref(self._h)), "mg_poseidon_create")

    @classmethod
    def decode(cls, curve, data, width=None, full_rounds=None, partial_rounds=None):
        """the manta codec of a `Hasher` (keys | MDS | tag, 32-byte canonical elements): the width follows from the length
        and the round counts from the width (manta-pay's specifications) unless given"""
        data = bytes(data)
        if width is None:
            fit = [w for w, (f, p) in POSEIDON_ROUNDS.items() if 32 * poseidon_param_count(w, f, p) == len(data)]
            if not fit:
                raise ValueError(f"{len(data)} bytes is no manta Poseidon parameter set of width 3..6")
            width = fit[0]
        f, p = POSEIDON_ROUNDS.get(width, (None, None))
        return cls(curve, width, f if full_rounds is None else full_rounds, p if partial_rounds is None else partial_rounds, data)

    def permute(self, states) -> np.ndarray:
        """[n, width, 4] states -> the permuted states (mg_poseidon_permute)"""
        st = np.array(_u64(states).reshape(-1, self.width, 4))
        _chk(LIB.mg_poseidon_permute(self._h, _p(st), st.shape[0]), "mg_poseidon_permute")
        return st

    def hash(self, inputs) -> np.ndarray:
        """[n, width - 1, 4] inputs -> [n, 4] digests (mg_poseidon_hash)"""
        x = _u64(inputs).reshape(-1, self.width - 1, 4)
        out = np.zeros((x.shape[0], 4), dtype=np.uint64)
        _chk(LIB.mg_poseidon_hash(self._h, _p(x), x.shape[0], _p(out)), "mg_poseidon_hash")
        return out

    def hash_device(self, d_inputs, n, d_out=None) -> "DeviceBuffer":
        """n x (width - 1) inputs already in HBM -> n digests in HBM (mg_poseidon_hash_device); d_out is allocated if None"""
        if d_out is None:
            d_out = DeviceBuffer(max(1, n) * 32)
        _chk(LIB.mg_poseidon_hash_device(self._h, _addr(d_inputs), n, _addr(d_out)), "mg_poseidon_hash_device")
        return d_out

    def close(self):
        if self._h is not None and self._h.value:
            LIB.mg_poseidon_destroy(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def merkle_tree(hasher: PoseidonHasher, height, leaves, indices=()):
    """`merkle_tree::Full` of `height` over the leaves (inserted left to right, [n, 4] Montgomery) with `hasher` (width 3) as
    the inner hash, on the GPU (mg_merkle_tree). Returns (root [4], paths [k, height - 1, 4]): manta's `Path` of each index --
    leaf sibling, then the inner siblings bottom-up, absent siblings 0."""
    lv = _u64(leaves).reshape(-1, 4)
    idx = np.ascontiguousarray(indices, dtype=np.uint64).reshape(-1)
    root = np.zeros(4, dtype=np.uint64)
    paths = np.zeros((idx.shape[0], max(0, int(height) - 1), 4), dtype=np.uint64)
    _chk(LIB.mg_merkle_tree(hasher._h, height, _p(lv), lv.shape[0], _p(root), _p(idx), idx.shape[0], _p(paths)), "mg_merkle_tree")
    return root, paths


def merkle_forest_roots(hasher: PoseidonHasher, height, leaves, offsets) -> np.ndarray:
    """roots of len(offsets) - 1 trees of `height` (mg_merkle_forest_roots): tree i holds leaves[offsets[i]:offsets[i + 1]]"""
    lv = _u64(leaves).reshape(-1, 4)
    off = np.ascontiguousarray(offsets, dtype=np.uint64).reshape(-1)
    nt = max(0, off.shape[0] - 1)
    roots = np.zeros((nt, 4), dtype=np.uint64)
    _chk(LIB.mg_merkle_forest_roots(hasher._h, height, _p(lv), _p(off), nt, _p(roots)), "mg_merkle_forest_roots")
    return roots


class _MerkleStateC(ctypes.Structure):  # mg_merkle_state
    _fields_ = [("counts", _vp), ("last_leaves", _vp), ("current_paths", _vp)]


class MerkleState:
    """what `mg_merkle_forest_append` knows a forest by (mg_merkle_state): per tree its leaf count, its last leaf and that
    leaf's `Path` -- `SinglePath` / `Partial::from_leaves_and_path` of the reference, the `CurrentPath`'s sentinels written
    out as zeros. counts [n_trees] uint64, last_leaves [n_trees, 4], current_paths [n_trees, height - 1, 4] (Montgomery)."""

    def __init__(self, counts, last_leaves, current_paths):
        self.counts = np.array(_u64(counts).reshape(-1))
        nt = self.counts.shape[0]
        self.last_leaves = np.array(_u64(last_leaves).reshape(nt, 4))
        cp = _u64(current_paths)
        self.current_paths = np.array(cp if cp.ndim == 3 and cp.shape[0] == nt else cp.reshape(nt, -1, 4))

    @classmethod
    def empty(cls, n_trees, height):
        """n_trees trees without leaves"""
        n_trees, height = int(n_trees), int(height)
        return cls(np.zeros(n_trees, dtype=np.uint64), np.zeros((n_trees, 4), dtype=np.uint64),
                   np.zeros((n_trees, max(0, height - 1), 4), dtype=np.uint64))

    @classmethod
    def from_tree(cls, leaves, path):
        """one tree from what `merkle_tree(hasher, height, leaves, indices=[n - 1])` was given and returned: its leaves (only
        their number and the last one are kept) and the paths array [1, height - 1, 4] (n = 0: any [0 or 1, height - 1, 4])"""
        lv = _u64(leaves).reshape(-1, 4)
        n, path = lv.shape[0], _u64(path)
        st = cls.empty(1, path.shape[-2] + 1)
        st.counts[0] = n
        if n:
            st.last_leaves[0], st.current_paths[0] = lv[-1], path.reshape(-1, 4)
        return st

    @classmethod
    def concat(cls, states):
        """the forest made of the trees of several states, in order"""
        states = list(states)
        return cls(np.concatenate([s.counts for s in states]), np.concatenate([s.last_leaves for s in states]),
                   np.concatenate([s.current_paths for s in states]))

    def __len__(self):
        return self.counts.shape[0]

    def _c(self):
        return _MerkleStateC(_p(self.counts), _p(self.last_leaves), _p(self.current_paths))


def merkle_forest_append(hasher: PoseidonHasher, height, state: MerkleState, leaves, offsets, path_requests=(), refresh=(),
                         in_place=False):
    """appends leaves[offsets[i]:offsets[i + 1]] to tree i of the forest `state` describes (mg_merkle_forest_append), without the
    older leaves. path_requests = (trees, indices) of new leaves whose `Path` in the new trees is wanted; refresh = (trees,
    indices, paths [m, height - 1, 4]) of older leaves whose `Path` in the old trees is brought up to date. Returns (roots
    [n_trees, 4], new state, paths [k, height - 1, 4], refreshed paths [m, height - 1, 4]). in_place: the new state is written
    over `state` (which is also returned)."""
    height = int(height)
    lv = _u64(leaves).reshape(-1, 4)
    off = np.ascontiguousarray(offsets, dtype=np.uint64).reshape(-1)
    nt, plen = len(state), max(0, height - 1)
    if off.shape[0] != nt + 1 or state.current_paths.shape[1] != plen:
        raise ValueError("offsets must have one entry more than the state has trees, and the state's paths height - 1 entries")
    pt, pi = (_u64(x).reshape(-1) for x in path_requests) if len(path_requests) else (np.zeros(0, dtype=np.uint64),) * 2
    if len(refresh):
        rt, ri = _u64(refresh[0]).reshape(-1), _u64(refresh[1]).reshape(-1)
        rp = np.array(_u64(refresh[2]).reshape(rt.shape[0], plen, 4))
    else:
        rt = ri = np.zeros(0, dtype=np.uint64)
        rp = np.zeros((0, plen, 4), dtype=np.uint64)
    if pt.shape != pi.shape or rt.shape != ri.shape:
        raise ValueError("a request is a (tree, index) pair")
    new = state if in_place else MerkleState.empty(nt, height)
    roots = np.zeros((nt, 4), dtype=np.uint64)
    paths = np.zeros((pt.shape[0], plen, 4), dtype=np.uint64)
    old_c, new_c = state._c(), new._c()
    _chk(LIB.mg_merkle_forest_append(hasher._h, height, nt, ctypes.byref(old_c), _p(lv), _p(off), _p(roots), ctypes.byref(new_c),
                                     _p(pt), _p(pi), pt.shape[0], _p(paths), _p(rt), _p(ri), rt.shape[0], _p(rp)),
         "mg_merkle_forest_append")
    return roots, new, paths, rp


def merkle_append(hasher: PoseidonHasher, height, state: MerkleState, leaves, path_indices=(), refresh=()):
    """merkle_forest_append for one tree: refresh = (indices, paths). Returns (root [4], new state, paths, refreshed paths)."""
    lv = _u64(leaves).reshape(-1, 4)
    pi = _u64(path_indices).reshape(-1)
    req = (np.zeros_like(pi), pi) if pi.shape[0] else ()
    ref = (np.zeros(len(refresh[0]), dtype=np.uint64), refresh[0], refresh[1]) if len(refresh) else ()
    roots, new, paths, rp = merkle_forest_append(hasher, height, state, lv, [0, lv.shape[0]], req, ref)
    return roots[0], new, paths, rp


# ---- manta-pay's embedded curve (ed_on_bn254) and its Poseidon note encryption -------------------------------------------
EDWARDS_CHUNK = 1 << 16  # MG_EDWARDS_CHUNK: lanes per device pass
EDWARDS_ORDER = 2736030358979909402780800718157159386076813972158567259200215660948447373041  # l, the subgroup order
EDWARDS_MUL_SHARED_SCALAR, EDWARDS_MUL_FIXED_BASE, EDWARDS_MUL_PAIRWISE = 0, 1, 2
NOTE_OK, NOTE_BAD_TAG, NOTE_BAD_VALUE, NOTE_OTHER_PARTITION = 0, 1, 2, 3
LIGHT_NOTE_BYTES, OUTGOING_NOTE_BYTES = 96, 64  # MG_LIGHT_NOTE_BYTES, MG_OUTGOING_NOTE_BYTES: ciphertext | tag


def _ed_points(points):
    return _u64(points).reshape(-1, 8)


def edwards_decode(data, checked=True, curve=BN254):
    """Batched ark-ec 0.3 `CanonicalDeserialize` of twisted Edwards points (`mg_edwards_decode`): data = 32-byte encodings back to
    back (or a sequence of them). Returns (points [n, 8] affine x | y Montgomery, identity (0, 1), zeros where rejected; status
    [n] uint8, POINT_*). checked=False skips only the subgroup test."""
    data = _joined(data)
    if len(data) % 32:
        raise ValueError(f"{len(data)} bytes is not a whole number of 32-byte encodings")
    n = len(data) // 32
    out = np.zeros((n, 8), dtype=np.uint64)
    st = np.zeros(n, dtype=np.uint8)
    _chk(LIB.mg_edwards_decode(curve, data, n, bool(checked), _p(out), _p(st), None), "mg_edwards_decode")
    return out, st


def edwards_encode(points, curve=BN254) -> bytes:
    """[n, 8] affine Montgomery points -> their 32-byte encodings back to back (`mg_edwards_encode`)"""
    pts = _ed_points(points)
    out = ctypes.create_string_buffer(max(1, pts.shape[0] * 32))
    _chk(LIB.mg_edwards_encode(curve, _p(pts), pts.shape[0], out), "mg_edwards_encode")
    return out.raw[:pts.shape[0] * 32]


def edwards_check(points, curve=BN254) -> np.ndarray:
    """status [n] uint8 (POINT_*) of affine Montgomery points: reduced, on the curve, in the subgroup (`mg_edwards_check`)"""
    pts = _ed_points(points)
    st = np.zeros(pts.shape[0], dtype=np.uint8)
    _chk(LIB.mg_edwards_check(curve, _p(pts), pts.shape[0], _p(st), None), "mg_edwards_check")
    return st


def edwards_scalars(values) -> np.ndarray:
    """Python integers -> [n, 4] uint64 canonical little-endian limbs"""
    return np.array([[(int(v) >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)] for v in values],
                    dtype=np.uint64).reshape(-1, 4)


def edwards_mul(mode, points, scalars, curve=BN254) -> np.ndarray:
    """`mg_edwards_mul`: EDWARDS_MUL_SHARED_SCALAR (n points x one scalar), EDWARDS_MUL_FIXED_BASE (one point x n scalars) or
    EDWARDS_MUL_PAIRWISE; points [., 8] affine Montgomery, scalars [., 4] canonical limbs below EDWARDS_ORDER -> [n, 8]"""
    pts, sc = _ed_points(points), _u64(scalars).reshape(-1, 4)
    n = pts.shape[0] if mode == EDWARDS_MUL_SHARED_SCALAR else sc.shape[0]
    out = np.zeros((n, 8), dtype=np.uint64)
    _chk(LIB.mg_edwards_mul(curve, mode, _p(pts), pts.shape[0], _p(sc), sc.shape[0], _p(out)), "mg_edwards_mul")
    return out


def edwards_add(a, b, curve=BN254) -> np.ndarray:
    """elementwise a[i] + b[i] of affine Montgomery points (`mg_edwards_add`)"""
    a, b = _ed_points(a), _ed_points(b)
    if a.shape != b.shape:
        raise ValueError("edwards_add: as many points in a as in b")
    out = np.zeros_like(a)
    _chk(LIB.mg_edwards_add(curve, _p(a), _p(b), a.shape[0], _p(out)), "mg_edwards_add")
    return out


class NoteCipher:
    """`IncomingBaseEncryptionScheme` (manta-pay/src/config/utxo.rs:744-758: `Hybrid` Diffie-Hellman over the embedded curve and
    `FixedDuplexer<1, Poseidon3>`) decoded from incoming-base-encryption-scheme.dat, with the group generator as an affine
    Montgomery point. Decoding is host-only; `encrypt` / `decrypt` run on the GPU, one note per lane."""

    def __init__(self, data, generator, curve=BN254):
        self._h = _vp()
        data = bytes(data)
        g = _u64(generator).reshape(-1)
        if g.size != 8:
            raise ValueError("generator: one affine point (8 x u64)")
        _chk(LIB.mg_note_cipher_create(curve, data, len(data), _p(g), ctypes.byref(self._h)), "mg_note_cipher_create")

    def encrypt(self, recv_keys, randomness, plaintexts):
        """n notes: recv_keys [n, 8], randomness [n, 4] scalars, plaintexts [n, 3, 4] Montgomery -> (epk [n, 8], ciphertext
        [n, 3, 4], tag [n, 4]) (`mg_notes_encrypt`)"""
        rk, rnd, pt = _ed_points(recv_keys), _u64(randomness).reshape(-1, 4), _u64(plaintexts).reshape(-1, 3, 4)
        n = rk.shape[0]
        if rnd.shape[0] != n or pt.shape[0] != n:
            raise ValueError("encrypt: one key, one randomness and one plaintext per note")
        epk, ct, tag = (np.zeros(s, dtype=np.uint64) for s in ((n, 8), (n, 3, 4), (n, 4)))
        _chk(LIB.mg_notes_encrypt(self._h, _p(rk), _p(rnd), _p(pt), n, _p(epk), _p(ct), _p(tag)), "mg_notes_encrypt")
        return epk, ct, tag

    def decrypt(self, viewing_key, epks, ciphertexts, tags):
        """n notes against one viewing key ([4] scalar) -> (plaintext [n, 3, 4], zeros where the note does not open; ok [n] bool;
        status [n] uint8 NOTE_*) (`mg_notes_decrypt`)"""
        vk, ep, ct, tg = _u64(viewing_key).reshape(-1), _ed_points(epks), _u64(ciphertexts).reshape(-1, 3, 4), _u64(tags).reshape(-1, 4)
        n = ep.shape[0]
        if vk.size != 4 or ct.shape[0] != n or tg.shape[0] != n:
            raise ValueError("decrypt: one viewing key; one epk, ciphertext and tag per note")
        pt = np.zeros((n, 3, 4), dtype=np.uint64)
        ok, st = np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.uint8)
        _chk(LIB.mg_notes_decrypt(self._h, _p(vk), _p(ep), _p(ct), _p(tg), n, _p(pt), _p(ok), _p(st)), "mg_notes_decrypt")
        return pt, ok.astype(bool), st

    def close(self):
        if self._h is not None and self._h.value:
            LIB.mg_note_cipher_destroy(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


UTXO_OK, UTXO_BAD_ENCODING, UTXO_MISMATCH = 0, 1, 2
SIGNATURE_MAX_MESSAGE = 1 << 16  # MG_SIGNATURE_MAX_MESSAGE: the largest stride of a message row
SIG_OK, SIG_BAD_ENCODING, SIG_DEGENERATE, SIG_MISMATCH = 0, 1, 2, 3


def _messages(messages, lengths, n):
    """[n, stride] uint8 rows and optional lengths [n] -> (rows, stride, lengths as uint32 or None)"""
    msg = np.ascontiguousarray(messages, dtype=np.uint8)
    if msg.ndim != 2 or msg.shape[0] != n:
        raise ValueError("messages: one row of `stride` bytes per signature")
    if lengths is not None:
        lengths = np.ascontiguousarray(lengths, dtype=np.uint32).reshape(-1)
        if lengths.shape[0] != n:
            raise ValueError("lengths: one per signature")
    return msg, msg.shape[1], lengths


class _UtxoFile(ctypes.Structure):
    _fields_ = [("bytes", ctypes.c_char_p), ("len", ctypes.c_size_t)]


class _UtxoFiles(ctypes.Structure):
    _fields_ = [(name, _UtxoFile) for name in ("utxo_commitment_scheme", "utxo_accumulator_item_hash",
                                               "nullifier_commitment_scheme", "viewing_key_derivation_function",
                                               "group_generator")]


class UtxoModel:
    """manta-pay's UTXO statement (manta-accounting/src/transfer/utxo/protocol.rs `derive_mint`, `utxo_check`, `item_hash`,
    `derive_spend`; manta-pay/src/config/utxo.rs) decoded from manta-parameters' utxo-commitment-scheme.dat,
    utxo-accumulator-item-hash.dat, nullifier-commitment-scheme.dat, viewing-key-derivation-function.dat and group-generator.dat
    (the files' bytes). Decoding is host-only; `mint` / `open` / `viewing_keys` run on the GPU, one UTXO or key per lane.
    Records are [n, 4, 4] (flag | public id | public value | commitment), plaintexts [n, 3, 4] (randomness | asset id | asset
    value), Montgomery limbs."""

    def __init__(self, utxo_commitment_scheme, utxo_accumulator_item_hash, nullifier_commitment_scheme,
                 viewing_key_derivation_function, group_generator, curve=BN254):
        self._h = _vp()
        self._files = [bytes(b) for b in (utxo_commitment_scheme, utxo_accumulator_item_hash, nullifier_commitment_scheme,
                                          viewing_key_derivation_function, group_generator)]
        files = _UtxoFiles(*[_UtxoFile(b, len(b)) for b in self._files])
        _chk(LIB.mg_utxo_model_create(curve, ctypes.byref(files), ctypes.byref(self._h)), "mg_utxo_model_create")

    def mint(self, recv_keys, plaintexts, flags):
        """n outputs: recv_keys [n, 8], plaintexts [n, 3, 4] holding the whole asset, flags [n] uint8 (1 = transparent) ->
        (utxos [n, 4, 4], items [n, 4], status [n] uint8 UTXO_*; zeros where the status is not UTXO_OK) (`mg_utxos_mint`)"""
        rk, pt = _ed_points(recv_keys), _u64(plaintexts).reshape(-1, 3, 4)
        fl = np.ascontiguousarray(flags, dtype=np.uint8).reshape(-1)
        n = rk.shape[0]
        if pt.shape[0] != n or fl.shape[0] != n:
            raise ValueError("mint: one key, one plaintext and one flag per UTXO")
        utxos, items, st = np.zeros((n, 4, 4), dtype=np.uint64), np.zeros((n, 4), dtype=np.uint64), np.zeros(n, dtype=np.uint8)
        _chk(LIB.mg_utxos_mint(self._h, _p(rk), _p(pt), _p(fl), n, _p(utxos), _p(items), _p(st)), "mg_utxos_mint")
        return utxos, items, st

    def open(self, viewing_key, plaintexts, utxos, pak=None):
        """`utxo_check` of n opened notes against the ledger's records for the address viewing_key * G, then the items and --
        with pak, one affine point -- the nullifier commitments -> (status [n] uint8 UTXO_*, items [n, 4], nullifiers [n, 4] or
        None, n_ok) (`mg_utxos_open`)"""
        vk, pt, ut = _u64(viewing_key).reshape(-1), _u64(plaintexts).reshape(-1, 3, 4), _u64(utxos).reshape(-1, 4, 4)
        n = pt.shape[0]
        if vk.size != 4 or ut.shape[0] != n:
            raise ValueError("open: one viewing key; one plaintext and one record per UTXO")
        if pak is not None:
            pak = _u64(pak).reshape(-1)
            if pak.size != 8:
                raise ValueError("pak: one affine point (8 x u64)")
        st, items = np.zeros(n, dtype=np.uint8), np.zeros((n, 4), dtype=np.uint64)
        nul = None if pak is None else np.zeros((n, 4), dtype=np.uint64)
        n_ok = _sz(0)
        _chk(LIB.mg_utxos_open(self._h, _p(vk), _p(pak), _p(pt), _p(ut), n, _p(st), _p(items), _p(nul), ctypes.byref(n_ok)),
             "mg_utxos_open")
        return st, items, nul, int(n_ok.value)

    def viewing_keys(self, paks, recv_keys=True):
        """n proof authorization keys [n, 8] -> (viewing keys [n, 4] canonical limbs below EDWARDS_ORDER, receiving keys [n, 8]
        or None) (`mg_viewing_keys`)"""
        pk = _ed_points(paks)
        n = pk.shape[0]
        vks = np.zeros((n, 4), dtype=np.uint64)
        rks = np.zeros((n, 8), dtype=np.uint64) if recv_keys else None
        _chk(LIB.mg_viewing_keys(self._h, _p(pk), n, _p(vks), _p(rks)), "mg_viewing_keys")
        return vks, rks

    def schnorr_challenges(self, pks, nonce_points, messages, lengths=None):
        """h = Blake2s-256(tag | enc(pk) | enc(R) | message) mod l of n signatures: pks, nonce_points [n, 8], messages [n, stride]
        uint8 with optional lengths [n] -> [n, 4] canonical limbs below EDWARDS_ORDER (`mg_schnorr_challenges`)"""
        pk, rp = _ed_points(pks), _ed_points(nonce_points)
        n = pk.shape[0]
        if rp.shape[0] != n:
            raise ValueError("schnorr_challenges: one key and one nonce point per signature")
        msg, stride, lens = _messages(messages, lengths, n)
        out = np.zeros((n, 4), dtype=np.uint64)
        _chk(LIB.mg_schnorr_challenges(self._h, _p(pk), _p(rp), _p(msg), stride, _p(lens), n, _p(out)), "mg_schnorr_challenges")
        return out

    def verify_signatures(self, pks, nonce_points, scalars, messages, lengths=None):
        """the ledger's `VerifySignature::verify` of n signatures (scalars [n, 4], nonce_points [n, 8]) under pks [n, 8] ->
        (status [n] uint8 SIG_*, n_ok) (`mg_signatures_verify`)"""
        pk, rp, sc = _ed_points(pks), _ed_points(nonce_points), _u64(scalars).reshape(-1, 4)
        n = pk.shape[0]
        if rp.shape[0] != n or sc.shape[0] != n:
            raise ValueError("verify_signatures: one key, one nonce point and one scalar per signature")
        msg, stride, lens = _messages(messages, lengths, n)
        st = np.zeros(n, dtype=np.uint8)
        n_ok = _sz(0)
        _chk(LIB.mg_signatures_verify(self._h, _p(pk), _p(rp), _p(sc), _p(msg), stride, _p(lens), n, _p(st),
                                      ctypes.byref(n_ok)), "mg_signatures_verify")
        return st, int(n_ok.value)

    def sign(self, signing_keys, nonces, messages, lengths=None, pks=True):
        """n signatures with the caller's keys and nonces ([n, 4] canonical limbs below EDWARDS_ORDER) -> (scalars [n, 4], nonce
        points [n, 8], verifying keys [n, 8] or None) (`mg_signatures_sign`)"""
        sk, k = _u64(signing_keys).reshape(-1, 4), _u64(nonces).reshape(-1, 4)
        n = sk.shape[0]
        if k.shape[0] != n:
            raise ValueError("sign: one key and one nonce per signature")
        msg, stride, lens = _messages(messages, lengths, n)
        s, rp = np.zeros((n, 4), dtype=np.uint64), np.zeros((n, 8), dtype=np.uint64)
        pk = np.zeros((n, 8), dtype=np.uint64) if pks else None
        _chk(LIB.mg_signatures_sign(self._h, _p(sk), _p(k), _p(msg), stride, _p(lens), n, _p(s), _p(rp), _p(pk)),
             "mg_signatures_sign")
        return s, rp, pk

    def address_partitions(self, recv_keys) -> np.ndarray:
        """`AddressPartitionFunction::partition` of n receiving keys [n, 8] -> [n] uint8 (`mg_address_partitions`)"""
        rk = _ed_points(recv_keys)
        out = np.zeros(rk.shape[0], dtype=np.uint8)
        _chk(LIB.mg_address_partitions(self._h, _p(rk), rk.shape[0], _p(out)), "mg_address_partitions")
        return out

    def light_encrypt(self, recv_keys, randomness, plaintexts, epks=True):
        """the AES-GCM light notes of n outputs: recv_keys [n, 8], randomness [n, 4] scalars, plaintexts [n, 3, 4] Montgomery ->
        (epk [n, 8] or None, notes [n, LIGHT_NOTE_BYTES] uint8 ciphertext | tag, status [n] uint8 NOTE_*; zeros where the
        status is not NOTE_OK) (`mg_light_notes_encrypt`)"""
        rk, rnd, pt = _ed_points(recv_keys), _u64(randomness).reshape(-1, 4), _u64(plaintexts).reshape(-1, 3, 4)
        n = rk.shape[0]
        if rnd.shape[0] != n or pt.shape[0] != n:
            raise ValueError("light_encrypt: one key, one randomness and one plaintext per note")
        epk = np.zeros((n, 8), dtype=np.uint64) if epks else None
        ct, st = np.zeros((n, LIGHT_NOTE_BYTES), dtype=np.uint8), np.zeros(n, dtype=np.uint8)
        _chk(LIB.mg_light_notes_encrypt(self._h, _p(rk), _p(rnd), _p(pt), n, _p(epk), _p(ct), _p(st)), "mg_light_notes_encrypt")
        return epk, ct, st

    def light_open(self, viewing_key, epks, notes, partitions=None):
        """`NoteOpen::open` of n light notes [n, LIGHT_NOTE_BYTES] against one viewing key ([4] scalar); with partitions [n] uint8
        only the notes that carry the byte of viewing_key * G are tried -> (plaintext [n, 3, 4], zeros where the note does not
        open; ok [n] bool; status [n] uint8 NOTE_*; n_tried) (`mg_light_notes_open`)"""
        vk, ep = _u64(viewing_key).reshape(-1), _ed_points(epks)
        ct = np.ascontiguousarray(notes, dtype=np.uint8).reshape(-1, LIGHT_NOTE_BYTES)
        n = ep.shape[0]
        if vk.size != 4 or ct.shape[0] != n:
            raise ValueError("light_open: one viewing key; one epk and one note per lane")
        if partitions is not None:
            partitions = np.ascontiguousarray(partitions, dtype=np.uint8).reshape(-1)
            if partitions.shape[0] != n:
                raise ValueError("partitions: one byte per note")
        pt = np.zeros((n, 3, 4), dtype=np.uint64)
        ok, st = np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.uint8)
        tried = _sz(0)
        _chk(LIB.mg_light_notes_open(self._h, _p(vk), _p(ep), _p(ct), _p(partitions), n, _p(pt), _p(ok), _p(st),
                                     ctypes.byref(tried)), "mg_light_notes_open")
        return pt, ok.astype(bool), st, int(tried.value)

    def outgoing_encrypt(self, recv_key, randomness, assets):
        """the outgoing notes of n spends, sealed to the spender's own receiving key ([8], one): randomness [n, 4] scalars,
        assets [n, 2, 4] Montgomery (id | value) -> (epk [n, 8], notes [n, OUTGOING_NOTE_BYTES] uint8, status [n] uint8 NOTE_*)
        (`mg_outgoing_notes_encrypt`)"""
        rk, rnd, a = _u64(recv_key).reshape(-1), _u64(randomness).reshape(-1, 4), _u64(assets).reshape(-1, 2, 4)
        n = rnd.shape[0]
        if rk.size != 8 or a.shape[0] != n:
            raise ValueError("outgoing_encrypt: one receiving key; one randomness and one asset per note")
        epk, ct, st = np.zeros((n, 8), dtype=np.uint64), np.zeros((n, OUTGOING_NOTE_BYTES), dtype=np.uint8), np.zeros(n, dtype=np.uint8)
        _chk(LIB.mg_outgoing_notes_encrypt(self._h, _p(rk), _p(rnd), _p(a), n, _p(epk), _p(ct), _p(st)),
             "mg_outgoing_notes_encrypt")
        return epk, ct, st

    def outgoing_open(self, viewing_key, epks, notes):
        """`NullifierOpen::open` of n outgoing notes [n, OUTGOING_NOTE_BYTES] against one viewing key -> (assets [n, 2, 4], zeros
        where the note does not open; ok [n] bool; status [n] uint8 NOTE_*) (`mg_outgoing_notes_open`)"""
        vk, ep = _u64(viewing_key).reshape(-1), _ed_points(epks)
        ct = np.ascontiguousarray(notes, dtype=np.uint8).reshape(-1, OUTGOING_NOTE_BYTES)
        n = ep.shape[0]
        if vk.size != 4 or ct.shape[0] != n:
            raise ValueError("outgoing_open: one viewing key; one epk and one note per lane")
        a = np.zeros((n, 2, 4), dtype=np.uint64)
        ok, st = np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.uint8)
        _chk(LIB.mg_outgoing_notes_open(self._h, _p(vk), _p(ep), _p(ct), n, _p(a), _p(ok), _p(st)), "mg_outgoing_notes_open")
        return a, ok.astype(bool), st

    def close(self):
        if self._h is not None and self._h.value:
            LIB.mg_utxo_model_destroy(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def merkle_shard_indices(leaves, curve=BN254) -> np.ndarray:
    """the shard of the UTXO Merkle forest each of n leaves [n, 4] (Montgomery) belongs to -> [n] uint8: what a caller sorts the
    leaves by to build the `offsets` of merkle_forest_roots (`mg_merkle_shard_indices`)"""
    lv = _u64(leaves).reshape(-1, 4)
    out = np.zeros(lv.shape[0], dtype=np.uint8)
    _chk(LIB.mg_merkle_shard_indices(curve, _p(lv), lv.shape[0], _p(out)), "mg_merkle_shard_indices")
    return out


class VerifyingContext:
    """Mirror of groth16::VerifyingContext<E> (manta-crypto/src/arkworks/groth16.rs:305-539): the prepared verifying key,
    resident on the GPU."""

    def __init__(self, curve, vk):
        """`VerifyingContext::new(&vk)`: vk = object with alpha_g1, beta_g2, gamma_g2, delta_g2, gamma_abc_g1 (affine
        Montgomery limb arrays) -- e.g. a ProvingKey."""
        self.curve = curve
        arrs = [_u64(getattr(vk, k)) for k in ("alpha_g1", "beta_g2", "gamma_g2", "delta_g2", "gamma_abc_g1")]
        h = _vp()
        _chk(LIB.mg_vk_create(curve, *[_p(a) for a in arrs], arrs[4].reshape(-1, affine_limbs(curve, 1)).shape[0], ctypes.byref(h)),
             "mg_vk_create")
        self.handle = h

    @classmethod
    def from_proving_context_key(cls, curve, pk):
        return cls(curve, pk)

    @classmethod
    def decode(cls, curve, data: bytes):
        self = cls.__new__(cls)
        self.curve = curve
        h = _vp()
        _chk(LIB.mg_vk_create_from_bytes(curve, bytes(data), len(data), ctypes.byref(h)), "mg_vk_create_from_bytes")
        self.handle = h
        return self

    def encode(self) -> bytes:
        out = ctypes.create_string_buffer(LIB.mg_vk_encoded_size(self.handle))
        _chk(LIB.mg_vk_encode(self.handle, out), "mg_vk_encode")
        return out.raw

    @property
    def num_inputs(self):
        return int(LIB.mg_vk_num_inputs(self.handle))

    def alpha_g1_beta_g2(self) -> bytes:
        out = ctypes.create_string_buffer(12 * FQ_LIMBS[self.curve] * 8)
        _chk(LIB.mg_vk_alpha_beta(self.handle, out), "mg_vk_alpha_beta")
        return out.raw

    def close(self):
        if getattr(self, "handle", None) is not None:
            LIB.mg_vk_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _proof_points(curve, proof):
    return proof_decode(curve, proof) if isinstance(proof, (bytes, bytearray)) else _u64(proof)


def groth16_verify(context: VerifyingContext, inputs, proof) -> bool:
    """Mirror of `Groth16::verify(context, input, proof)` (groth16.rs:603-609): inputs = [P - 1, 4] Montgomery Fr,
    proof = the proof bytes (decoded and checked first) or its a | b | c limbs."""
    inp = _u64(inputs).reshape(-1, 4)
    if inp.shape[0] != context.num_inputs - 1:
        raise ValueError(f"{inp.shape[0]} public inputs, the key takes {context.num_inputs - 1}")
    ok = ctypes.c_int(0)
    pts = _proof_points(context.curve, proof)
    _chk(LIB.mg_groth16_verify(context.handle, _p(inp), _p(pts), ctypes.byref(ok)), "mg_groth16_verify")
    return bool(ok.value)


def groth16_verify_batch(context: VerifyingContext, inputs, proofs, rand128) -> bool:
    """k proofs of one key in one pass (`mg_groth16_verify_batch`): inputs [k, P - 1, 4], proofs = k proof byte strings
    (or [k, limbs] points), rand128 [k, 2] uint64: 128 random bits per proof (not both words zero; proof i enters with k1 + lambda k2, see mantagpu.h)."""
    k = len(proofs)
    inp = _u64(inputs).reshape(k, -1, 4)
    if inp.shape[1] != context.num_inputs - 1:
        raise ValueError("public-input count does not match the key")
    pts = np.stack([_proof_points(context.curve, p) for p in proofs])
    rnd = _u64(rand128).reshape(k, 2)
    ok = ctypes.c_int(0)
    _chk(LIB.mg_groth16_verify_batch(context.handle, k, _p(inp), _p(_u64(pts)), _p(rnd), ctypes.byref(ok)),
         "mg_groth16_verify_batch")
    return bool(ok.value)


VERIFY_EACH_CHUNK = 1024  # MG_VERIFY_EACH_CHUNK: proofs / pairing groups per device pass of the *_each calls


def _verdicts(n, out):
    """the byte array a *_each call writes its n verdicts to: the caller's (uint8, at least n) or a fresh one"""
    if out is None:
        return np.zeros(n, dtype=np.uint8)
    if out.dtype != np.uint8 or not out.flags.c_contiguous or out.size < n:
        raise ValueError("out: a contiguous uint8 array of at least one byte per verdict")
    return out


def groth16_verify_each(context: VerifyingContext, inputs, proofs, out=None) -> np.ndarray:
    """k proofs of one key, a verdict each (`mg_groth16_verify_each`): element i is what `groth16_verify` answers for
    (inputs[i], proofs[i]), in one pass over the block. inputs [k, P - 1, 4] (None or empty for a key without public inputs),
    proofs = k proof byte strings or [k, limbs] points. The verdicts are also written to `out` (uint8) when given."""
    k = len(proofs)
    n_in = context.num_inputs - 1
    inp = np.zeros((k, 0, 4), dtype=np.uint64) if inputs is None else _u64(inputs)
    if inp.size != k * n_in * 4:
        raise ValueError(f"{inp.size // 4} public inputs for {k} proofs, the key takes {n_in} each")
    inp = inp.reshape(k, n_in, 4)
    ok = _verdicts(k, out)
    pts = _u64(np.stack([_proof_points(context.curve, p) for p in proofs])) if k else np.zeros((0, 1), dtype=np.uint64)
    _chk(LIB.mg_groth16_verify_each(context.handle, k, _p(inp) if n_in and k else None, _p(pts) if k else None,
                                    _p(ok)), "mg_groth16_verify_each")
    return ok[:k].astype(bool)


def pairing_check_each(curve, g1_points, g2_points, out=None) -> np.ndarray:
    """n_groups independent `pairing_check`s in one pass (`mg_pairing_check_each`): g1_points [n_groups, group_size, 2 * limbs],
    g2_points [n_groups, group_size, 4 * limbs] affine Montgomery; element t says whether prod_j e(P[t][j], Q[t][j]) == 1."""
    g1, g2 = _u64(g1_points), _u64(g2_points)
    if g1.ndim != 3 or g2.ndim != 3 or g1.shape[:2] != g2.shape[:2] or g1.shape[2] != affine_limbs(curve, 1) or \
            g2.shape[2] != affine_limbs(curve, 2):
        raise ValueError("pairing_check_each: [n_groups, group_size, limbs] arrays, as many G1 as G2 points")
    n, g = g1.shape[:2]
    ok = _verdicts(n, out)
    _chk(LIB.mg_pairing_check_each(curve, _p(g1) if n else None, _p(g2) if n else None, g, n, _p(ok)), "mg_pairing_check_each")
    return ok[:n].astype(bool)
