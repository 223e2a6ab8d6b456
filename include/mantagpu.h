/* mantagpu.h -- C ABI of the MI355X-native Groth16 prove hot path (libmantagpu.so).
 *
 * This is the drop-in boundary for ONE path of Manta-Network/manta-rs: the body of
 *     manta_crypto::arkworks::groth16::Groth16::<E>::prove      (manta-crypto/src/arkworks/groth16.rs:589-600)
 * i.e. `ArkGroth16::prove(&context.proving_key, compiler, &mut SizedRng(rng))` and the arkworks 0.3
 * primitives underneath it (ark-ec VariableBaseMSM, ark-poly Radix2EvaluationDomain, ark-groth16
 * R1CStoQAP::witness_map + create_proof). Everything else in manta-rs keeps calling arkworks.
 * INTEGRATION.md shows the Rust `extern "C"` block and the replacement body of `prove`.
 *
 * Conventions (same as arkworks' in-memory data, so the Rust side passes slices without conversion):
 *   - field element  = little-endian u64 limbs (4 for Fr and BN254 Fq, 6 for BLS12-381 Fq), Montgomery
 *     form with R = 2^(64*limbs)  [ark-ff Fp256/Fp384 `.0.0`]
 *   - MSM scalars    = 4 x u64 canonical integers [`Fr::into_repr()`], unless a call says "mont"
 *   - affine point   = x || y (G2: x.c0 x.c1 y.c0 y.c1); infinity = all limbs zero (the shim writes
 *     zeros for `GroupAffine{infinity: true}`; (0,0) is never on either curve)
 *   - proof bytes    = arkworks canonical compressed A || B || C (128 B BN254, 192 B BLS12-381),
 *     byte-identical to `proof_as_bytes` (manta-crypto/src/arkworks/groth16.rs:186-195)
 *   - every function returns 0 on success; any non-zero maps to the reference's opaque unit `Error`
 *     (groth16.rs:50-60). No exceptions, no abort. mg_strerror()/mg_last_error() give detail.
 *   - objects belong to the HIP device current at creation (or to the devices of the list a `_sharded`
 *     constructor was given) and remember it: calls on them may come from any thread, whatever that
 *     thread's current device. One process per GPU (torch.distributed / RCCL between them) and one process
 *     driving several GPUs (the `_sharded` entry points) are both supported.
 *   - all entry points are re-entrant; `mg_groth16_prove` may be called concurrently on one context (the
 *     reference's `prove` takes `&ProvingContext`, groth16.rs:589-596). `mg_ctx_set_r1cs` is the one mutator:
 *     it waits for the proofs in flight on the context, and proofs that start later see the new circuit.
 *   - the library never retains host pointers after a call returns.
 */
#ifndef MANTAGPU_H
#define MANTAGPU_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum { MG_BN254 = 0, MG_BLS12_381 = 1 } mg_curve_t;

enum {
    MG_SUCCESS = 0,
    MG_ERROR_INVALID_ARGUMENT = 1,
    MG_ERROR_HIP = 2,
    MG_ERROR_OUT_OF_MEMORY = 3,
    MG_ERROR_DOMAIN_TOO_LARGE = 4, /* ark-relations SynthesisError::PolynomialDegreeTooLarge */
    MG_ERROR_STATE = 5,
    MG_ERROR_CHECKSUM = 6 /* the BLAKE3 digest of the data does not match (mg_ctx_create_from_bytes_checked) */
};

typedef struct mg_bases mg_bases;     /* a static vector of curve points resident in HBM */
typedef struct mg_msm_job mg_msm_job; /* an MSM in flight */
typedef struct mg_ctx mg_ctx;         /* device-resident ProvingContext (+ R1CS matrices) */

/* ---- runtime ---------------------------------------------------------------------------------- */
int mg_init(int device);                /* hipSetDevice + engine warm-up; optional */
const char *mg_strerror(int status);
const char *mg_last_error(void);        /* thread-local detail of the last failure */
int mg_device_count(int *count);
/* Raw HBM buffers, for hosts without a HIP binding (tests, bench). */
int mg_malloc(void **dptr, size_t bytes);
int mg_free(void *dptr);
/* DEVICE INPUTS MUST BE COMPLETE BEFORE THE CALL. The two copies below, mg_ntt_device, mg_fixed_base_mul and mg_field_op run on a
 * NON-blocking stream of the library's and wait for that stream alone: they do not order themselves against the host's default
 * (NULL) stream or any other. A caller whose own kernels or copies produced a device input synchronises them first; the
 * output is complete when the call returns. */
int mg_memcpy_h2d(void *dptr, const void *hptr, size_t bytes);
int mg_memcpy_d2h(void *hptr, const void *dptr, size_t bytes); /* (dptr: complete before the call, see above) */
int mg_device_synchronize(void);
/* Page-locked host memory. An assignment (`z_mont`) that lives in a buffer from mg_host_alloc -- or in any
 * memory the caller registered with HIP -- is DMA'd to the GPU straight from where it is; any other buffer is
 * first copied into the library's own pinned staging area (0.1 ms for the 1.1 MB PrivateTransfer assignment). The
 * Rust shim can collect `instance || witness` directly into such a buffer. */
int mg_host_alloc(void **hptr, size_t bytes);
int mg_host_free(void *hptr);
/* Measurement hook (bench.py roofline leg): when on, each MSM brackets its dominant kernel (bucket
 * accumulate) with HIP events on the stream it is launched on; mg_last_accumulate_ms() returns the
 * duration of the calling thread's most recently finished MSM. Off by default. */
int mg_set_kernel_timing(int on);
float mg_last_accumulate_ms(void);
float mg_last_accumulate_mhz(void); /* the shader clock that launch ran at: s_memtime ticks of its first wavefront per wall-clock second */
/* With kernel timing on, the same for the calling thread's last mg_ntt / mg_ntt_device -- out4 = { whole call on the device,
 * conversion in, butterfly passes, conversion out } in ms -- and for its last SINGLE proof, which is then enqueued with plain
 * launches instead of the captured graphs -- out10 = { upload of z, witness map, MSM a, b_g1, b_g2, l, h (each on its own
 * stream), part A (all but the G2 MSM) from upload to join, the G2 chain from upload to its end, host assembly after the
 * GPU } in ms: the per-phase report SURVEY.md 8(d) asks of BASELINE configs[2]. */
/* Clock probe: two wavefronts per SIMD on every CU spin on dependent v_mad_u64_u32 chains (the instruction the MSM is
 * bound by) for `iters` x 32 multiply-adds each, reading the shader clock counter (s_memtime) and the constant-rate wall
 * clock around the loop: *memtime_mhz = the rate the counter ran at under that load, *mad_issue_per_us_per_simd = wave-level
 * multiply-adds a SIMD issued per microsecond (the measured issue peak, no clock assumed), *ms = duration of the probe. */
int mg_clock_probe(unsigned iters, double *memtime_mhz, double *mad_issue_per_us_per_simd, double *ms);
int mg_last_ntt_ms(float out4[4]);
int mg_last_prove_phases_ms(float out10[10]);
/* Always on (three clock reads per pass): the HOST side of the calling thread's last proving pass on an unsharded context --
 * out3 = { staging z and enqueuing the pass (graph launches or ~100 kernel launches), waiting for the GPU, assembly after the
 * last MSM result arrived } in ms. A pass whose first figure approaches its wall time is bound by launches, not by kernels. */
int mg_last_pass_host_ms(float out3[3]);
/* Introspection: the hardware queues the library found behind the current device's streams -- out2 = { normal priority, high
 * priority }, 0 / 0 before the first proving context with queue_aware = 1 exists. The HIP runtime multiplexes streams onto a
 * few hardware queues per priority level and kernels of streams that share one run one behind the other; the library measures the
 * sharing once per device (csrc/queues.hip) and gives every single-proof slot three streams on three different queues. */
int mg_hw_queues(int out2[2]);

/* ---- variable-base MSM: replaces ark_ec::msm::VariableBaseMSM::multi_scalar_mul(bases, scalars)
 *      (ark-ec 0.3.0 msm/variable_base.rs; called 5x per proof from ark-groth16 create_proof, reached
 *      from manta-crypto/src/arkworks/groth16.rs:597) ------------------------------------------------ */
/* Register `n` affine points (host pointer, or device pointer if on_device). group = 1 (G1) or 2 (G2).
 * precompute_window_bits > 0 additionally stores 2^(c*w)*P for every window (HBM for speed: all
 * windows then share one bucket set and no doubling chain remains); 0 = plain bases;
 * -12 .. -2 = FULL tables of window width c = -precompute_window_bits: every multiple m*2^(c*w)*P, m = 1 .. 2^(c-1), so
 * that a signed digit addresses its summand and the MSM is one plain sum (no buckets, no sort, no bucket reduce) --
 * ceil(bits/c) * 2^(c-1) points per base, fewer than 2^31 in all, for fixed proving-key queries of proof size. */
int mg_bases_create(mg_curve_t curve, int group, const uint64_t *affine_mont, size_t n, int on_device,
                    int precompute_window_bits, mg_bases **out);
/* The same vector range-sharded over a list of devices ("MSM shards by scalar/base
 * range across the GPUs of one node"): shard g = points [n*g/G, n*(g+1)/G) on devices[g], host pointer only. A
 * device may appear more than once (functional testing of the multi-GPU path on one GPU). */
int mg_bases_create_sharded(mg_curve_t curve, int group, const uint64_t *affine_mont, size_t n, const int *devices,
                            int n_devices, int precompute_window_bits, mg_bases **out);
int mg_bases_num_shards(const mg_bases *bases);
int mg_bases_shard(const mg_bases *bases, int shard, int *device, size_t *lo, size_t *hi);
void mg_bases_destroy(mg_bases *bases);
size_t mg_bases_device_bytes(const mg_bases *bases);
/* Host-to-host convenience: result = sum_i scalars[i] * bases[i], i < n <= len(bases).
 * scalars: n x 4 u64 canonical. out: affine Montgomery (infinity = zeros). */
int mg_msm(const mg_bases *bases, const uint64_t *scalars_canonical, size_t n, uint64_t *out_affine_mont);
/* Scalars already resident in HBM (the timed path). `scalar_flags`: MG_SCALARS_MONT -- the scalars are Montgomery Fr
 * and are converted on the device (`into_repr`), else canonical; MG_SCALARS_SPARSE -- a hint that many digits are
 * zero (a witness: mostly 0 / 1 / small values), the zero digits are then compacted away before the sort.
 * window_bits = 0 lets the library choose. Returns immediately; mg_msm_finish waits and writes the affine result. */
#define MG_SCALARS_MONT 1
#define MG_SCALARS_SPARSE 2
int mg_msm_launch(const mg_bases *bases, const uint64_t *d_scalars, size_t n, int scalar_flags, int window_bits,
                  mg_msm_job **job);
/* Sharded bases: d_scalars_per_shard[g] points at the scalars of shard g's range, resident on shard g's device.
 * One Pippenger pass per device, all in flight at once; the per-device partial points are the only data exchanged
 * and mg_msm_finish adds them. (mg_msm, the host-to-host call, accepts sharded bases too and uploads the slices.) */
int mg_msm_launch_sharded(const mg_bases *bases, const uint64_t *const *d_scalars_per_shard, int scalar_flags,
                          int window_bits, mg_msm_job **job);
int mg_msm_finish(mg_msm_job *job, uint64_t *out_affine_mont); /* waits, folds, adds the shards' partial points, frees the job */
/* The result of a job left on the DEVICE instead of the host: the window sums are folded by one more small kernel behind
 * the MSM (bases with precomputed multiples only, else MG_ERROR_STATE: plain bases end in a 255-doubling Horner chain,
 * a host job) and the point -- X | Y | ZZ | ZZZ in arkworks' Montgomery limbs, x = X/ZZ, y = Y/ZZZ, ZZ = 0 for infinity;
 * mg_xyzz_limbs() u64 -- is written to d_out_xyzz. `stream` (a hipStream_t; NULL = the default stream) is made to wait for it, so a
 * consumer on another stream -- the RCCL all_gather of the range-sharded MSM (partial points gathered
 * from device memory) -- needs no host synchronisation between launch and collective. The job is still released with
 * mg_msm_finish (out_affine_mont may be NULL). Single-shard jobs only. */
int mg_msm_result_to_device(mg_msm_job *job, uint64_t *d_out_xyzz, void *stream);
size_t mg_xyzz_limbs(mg_curve_t curve, int group); /* u64 per XYZZ point: 16 / 24 (G1), 32 / 48 (G2) */
/* sum of n XYZZ points (host memory, the layout above) -> one affine point: the N-term sum after the all_gather */
int mg_xyzz_sum(mg_curve_t curve, int group, const uint64_t *xyzz, size_t n, uint64_t *out_affine_mont);
/* sum of the registered points themselves (multi-GPU partial-point reduction, tests) */
int mg_points_sum(mg_curve_t curve, int group, const uint64_t *affine_mont, size_t n, uint64_t *out_affine_mont);
/* [k_i] * base for n canonical scalars in HBM -> n affine points in HBM (fixed-base batch multiply:
 * synthetic base generation; key generation as in ark-groth16 generate_parameters). d_scalars: complete before the call
 * (see mg_memcpy_h2d). */
int mg_fixed_base_mul(mg_curve_t curve, int group, const uint64_t *base_affine_mont, const uint64_t *d_scalars,
                      size_t n, uint64_t *d_out_affine_mont);
/* Element-wise group operations on host arrays of n affine points, computed on the GPU with the MSM kernels' own
 * device functions (mixed / general addition, doubling, double-and-add) and normalised with the batched
 * Montgomery-trick inversion -- the primitive menu the reference itself benchmarks and cross-checks
 * (manta-benchmark/src/ecc.rs:30-128, consistency tests :138-172):
 *   MG_EC_ADD_MIXED  out = a + b   `projective += affine`            (ecc.rs:69-74)
 *   MG_EC_ADD        out = a + b   `projective += projective`        (ecc.rs:78-83)
 *   MG_EC_DOUBLE     out = 2a      (b unused)
 *   MG_EC_MUL        out = [k]a    b = n x 4 u64 canonical scalars   (ecc.rs:87-101)
 *   MG_EC_SUB_MIXED  out = a - b
 * out = n affine points (batch normalisation, ecc.rs:114-119). */
#define MG_EC_ADD_MIXED 0
#define MG_EC_ADD 1
#define MG_EC_DOUBLE 2
#define MG_EC_MUL 3
#define MG_EC_SUB_MIXED 4
/*   MG_EC_MUL_FIXED  out = [k]a    b = ONE canonical scalar (4 u64) for all points: `batch_mul_fixed_scalar`
 *                                   (manta-trusted-setup/src/util.rs:440-445; Groth16 MPC `contribute`, mpc.rs:451-468);
 *   MG_EC_MUL with per-point scalars is `batch_mul_pointwise` (util.rs:447-455; kzg `Accumulator::update`, kzg.rs:444-468) */
#define MG_EC_MUL_FIXED 5
int mg_ec_elementwise(mg_curve_t curve, int group, int op, const uint64_t *a_affine, const uint64_t *b, size_t n,
                      uint64_t *out_affine);
/* Element-wise prime-field arithmetic on the GPU with the kernels' own device functions: the direct parity surface
 * for ark-ff 0.3 Fp256 / Fp384 (`ark_ff::Fp256<..>::{add_assign, sub_assign, mul_assign, square, neg, inverse, from_repr,
 * into_repr}`; re-exported manta-crypto/src/arkworks/mod.rs:25-35).
 *   field: 0 BN254 Fr, 1 BN254 Fq, 2 BLS12-381 Fr, 3 BLS12-381 Fq;  elements = 4 / 4 / 4 / 6 u64 limbs, Montgomery
 *          (MG_FIELD_FROM_CANONICAL takes, MG_FIELD_TO_CANONICAL returns, plain integers)
 *   repr:  0 = the saturated 32-bit-limb Montgomery arithmetic of the NTT / SpMV kernels (ABI format);
 *          1 = the reduced-radix lazily-reduced arithmetic inside the MSM kernels: a (b) is converted, lazy_a (lazy_b)
 *              in 0..3 times p is added so that the operation runs on a non-canonical representative, and the result
 *              comes back canonical. out[i] = a[i] op b[i]; b is ignored by the unary operations. */
#define MG_FIELD_ADD 0
#define MG_FIELD_SUB 1
#define MG_FIELD_MUL 2
#define MG_FIELD_SQR 3
#define MG_FIELD_NEG 4
#define MG_FIELD_FROM_CANONICAL 5
#define MG_FIELD_TO_CANONICAL 6
#define MG_FIELD_INV 7
/* a, b, out: device memory; a and b complete before the call (see mg_memcpy_h2d) */
int mg_field_op(int field, int op, int repr, int lazy_a, int lazy_b, const uint64_t *a, const uint64_t *b, size_t n,
                uint64_t *out);
/* The reduced-radix routines of the MSM kernels on RAW limb vectors: a, b, c, d and out are [n][K] uint32 limbs of LB bits
 * (K x LB = 9 x 29 for the three 256-bit fields, 13 x 30 for BLS12-381 Fq), used as they are -- no conversion before or after.
 *   op 0: a b R'^-1   1: a^2 R'^-1   2: (a b + c d) R'^-1   (almost-Montgomery, R' = 2^(K LB): the exact integer
 *         (t + (t (-p^-1) mod R') p) / R' of t = a b [+ c d], K - 1 masked limbs and the unmasked top limb)
 *      3: a + 6 p - b - 2 c   4: a + 12 p - b - 2 c   (limbs normalised; need b + 2 c < 6 p, 12 p)
 *   coding 0: the plain routines (mul, sqr, mul_add -- for BLS12-381 Fq one column walker for all three -- and sub2); 1: what the
 *   accumulate kernel calls (mul_t / sqr_t / mul_add_t<true>, sub2n). Coding 1 is the single-chain coding of the products for
 *   every field (asm links for the 29-bit fields; the same walker with its multiply-adds pinned in C for BLS12-381 Fq, where
 *   -DMG_CHAIN_FLUSHED=0 builds the three as the plain routines again: an A/B twin).
 * Operands an op does not take are ignored (may be NULL). n <= 2^24. */
#define MG_FPR_MUL 0
#define MG_FPR_SQR 1
#define MG_FPR_MUL_ADD 2
#define MG_FPR_SUB2_6 3
#define MG_FPR_SUB2_12 4
int mg_fpr_raw_op(int field, int op, int coding, const uint32_t *a, const uint32_t *b, const uint32_t *c, const uint32_t *d,
                  size_t n, uint32_t *out);
/* Where those products move a column accumulator's upper part aside ("flush") so that it cannot pass 2^64 -- the compile-time
 * plan of the kernels, readable without a GPU. kind = MG_FPR_MUL / MG_FPR_SQR / MG_FPR_MUL_ADD. flush[k], k < 2 K - 1:
 * bit 0 / 1 / 2 = flush before the a b / c d / m p products of column k; peak[k] = the planner's worst-case accumulator value
 * of the column. *cols = 2 K - 1 (flush and peak hold at least 25 entries), *limb_bits = LB, *flushed_routines = 1 when the
 * field's plans hold a flush at all (its products then walk their columns by the plan). Any output may be NULL. */
int mg_fpr_column_plan(int field, int kind, uint32_t *flush, uint64_t *peak, int *cols, int *limb_bits, int *flushed_routines);
/* The first two stages of the MSM pipeline, each alone over host arrays: parity-test surfaces for the kernels that
 * mg_msm_launch runs (the same digit kernel, the same radix sort), not needed by the shim. Synchronous; one device
 * block per call. The OUTPUT arrays are uploaded from the caller's buffers before the launch, so whatever the kernels
 * do not write comes back as the caller left it.
 *
 * mg_msm_digits: scalars [batch][n_scalars][4] u64 (canonical integers of any size below 2^256, or Montgomery words
 *   with MG_SCALARS_MONT) -> signed window digits -> (bucket key, base index | sign << 31) pairs for a set of n stored
 *   bases that is described, not supplied: table_mode 0 = plain bases, 1 = a table per window, 2 = full tables
 *   (window_bits 2..12); map = NULL or n indices (stored base i takes scalar map[i]); the set is the concatenation of
 *   n_sets queries of set_len entries (n_sets = 1: set_len = its logical length; n = n_sets * set_len without a map,
 *   n_scalars <= set_len for n_sets > 1). Stored bases without a scalar (index >= n_scalars) have the scalar 0.
 *   layout = {W = ceil(scalar bits / window_bits), B = 2^(window_bits - 1), bucket keys per (vector, query), the key
 *   of a zero digit}. keys, vals: batch * W * n u32 each. compact = 0: digit (vector q, window w, base i) at
 *   (q W + w) n + i, zero digits as (invalid key, 0). compact = 1: the pairs of the non-zero digits only, in an
 *   unspecified order at the front of the arrays, their number in *count.
 *   MG_ERROR_INVALID_ARGUMENT for what an MSM launch refuses: 2^31 pairs, a key space of 2^24 (batch * n_sets *
 *   bucket keys), a base index of 2^31, index ranges that contradict each other.
 * mg_sort_pairs: n (key, value) pairs, keys below 2^end_bit (1 <= end_bit <= 32; the caller's duty), sorted stably by
 *   key. count != NULL: only the first *count <= n pairs exist (the number is read on the device) and the outputs from
 *   *count on are not written. (lowmask, inv_from) = (0xffffffff, 0xffffffff): the key itself; otherwise the order is
 *   that of key >= inv_from ? lowmask + 1 : key & lowmask, which must be below 2^end_bit. */
int mg_msm_digits(mg_curve_t curve, const uint64_t *scalars, size_t batch, size_t n_scalars, int scalar_flags, int window_bits,
                  int table_mode, size_t n, const uint32_t *map, size_t n_sets, size_t set_len, int compact, uint32_t *keys,
                  uint32_t *vals, uint32_t *count, uint32_t layout[4]);
int mg_sort_pairs(const uint32_t *keys, const uint32_t *vals, size_t n, int end_bit, const uint32_t *count, uint32_t lowmask,
                  uint32_t inv_from, uint32_t *keys_out, uint32_t *vals_out);
/* The fused front end a stand-alone MSM takes where mg_msm_dense_front_applies: both stages as one, no unsorted pairs in memory.
 * mg_msm_dense_front_applies: 1 if a launch of `batch` scalar vectors over a set of n_sets queries with `windows` windows and
 *   the given table_mode (as above), compaction asked for (MG_SCALARS_SPARSE) or not, has the shape for it, else 0. A pure
 *   function: no device is touched.
 * mg_msm_dense_front: one vector of n_scalars scalars against n stored bases with a table per window -> the W * n pairs of ALL
 *   digits SORTED by key in keys / vals (uploaded first, as above). A zero digit is the pair (key 0, layout[3]): layout =
 *   {W, B, bucket keys, the index of the infinity record behind the last table = W * n}. The order inside a run of equal keys
 *   is unspecified. MG_ERROR_INVALID_ARGUMENT for a shape mg_msm_dense_front_applies turns down and for what a launch refuses. */
int mg_msm_dense_front_applies(size_t batch, size_t n_sets, int windows, int table_mode, int sparse);
int mg_msm_dense_front(mg_curve_t curve, const uint64_t *scalars, size_t n_scalars, int scalar_flags, int window_bits, size_t n,
                       const uint32_t *map, size_t set_len, uint32_t *keys, uint32_t *vals, uint32_t layout[4]);
/* Radix-2 (inverse) NTT over a vector of 2^log_n GROUP elements, natural order in and out: ark-poly
 * `Radix2EvaluationDomain::{fft, ifft}` applied to points -- how `mpc::initialize` turns the powers of tau into the
 * Lagrange basis (manta-trusted-setup/src/groth16/mpc.rs:378-381). Host arrays of affine Montgomery points. */
int mg_group_ntt(mg_curve_t curve, int group, const uint64_t *points_affine, unsigned log_n, int inverse, uint64_t *out_affine);
/* arkworks canonical serialisation of one affine point (compressed: 32/48/64/96 B) */
int mg_point_serialize(mg_curve_t curve, int group, const uint64_t *affine_mont, int compressed, uint8_t *out);

/* ---- radix-2 NTT over Fr: replaces ark_poly::Radix2EvaluationDomain::{fft,ifft,coset_fft,
 *      coset_ifft}_in_place (ark-poly 0.3.0; used 7x per proof by R1CStoQAP::witness_map) ------------ */
/* data: 2^log_n Montgomery Fr elements, natural order in and out, transformed in place. */
int mg_ntt(mg_curve_t curve, uint64_t *data_mont, unsigned log_n, int inverse, int coset);
/* the same on data resident in HBM, which must be complete before the call (see mg_memcpy_h2d) */
int mg_ntt_device(mg_curve_t curve, uint64_t *d_data_mont, unsigned log_n, int inverse, int coset);

/* ---- Groth16 proving context: replaces ProvingContext<E>{proving_key} (groth16.rs:216-245) +
 *      ark_groth16::create_proof ----------------------------------------------------------------------- */
typedef struct {
    uint64_t n_vars;   /* V: instance + witness variables (len of a_query) */
    uint64_t n_inputs; /* P: instance variables incl. the constant one */
    uint64_t h_len;    /* len(h_query): D-1 (ark setup) or D (MPC keys, mpc.rs:372-377) */
    const uint64_t *alpha_g1, *beta_g1, *delta_g1; /* G1 affine */
    const uint64_t *beta_g2, *delta_g2;            /* G2 affine */
    const uint64_t *a_query;    /* V   x G1 */
    const uint64_t *b_g1_query; /* V   x G1 */
    const uint64_t *b_g2_query; /* V   x G2 */
    const uint64_t *h_query;    /* h_len x G1 */
    const uint64_t *l_query;    /* V-P x G1 */
} mg_pk_view;

typedef struct {
    const uint32_t *row_ptr; /* m+1 */
    const uint32_t *col;     /* nnz  */
    const uint64_t *val;     /* nnz x 4, Montgomery Fr */
    uint64_t nnz;
} mg_csr;

/* ---- key generation: the expensive part of `Groth16::compile` (manta-crypto/src/arkworks/groth16.rs:571-586 ->
 *      ark-groth16 0.3 generate_parameters): every group element of the proving and verifying key is a fixed-base
 *      multiple of a generator, 3V + D of them in G1 and V in G2 -- computed on the GPU. The caller supplies what
 *      the reference draws from its RNG, in its order: alpha, beta, gamma, delta (then the two generators), tau --
 *      all Fr in Montgomery form -- so a seeded RNG reproduces the reference's key. Outputs are caller-allocated
 *      arrays laid out like the fields of the mg_pk_view struct -- affine Montgomery, infinity = zeros: gamma_abc_g1[n_inputs],
 *      a_query / b_g1_query / b_g2_query[n_vars], h_query[D - 1] with D = next_pow2(m + n_inputs),
 *      l_query[n_vars - n_inputs]. */
typedef struct mg_pk_out {
    uint64_t *alpha_g1, *beta_g1, *delta_g1;
    uint64_t *beta_g2, *gamma_g2, *delta_g2;
    uint64_t *gamma_abc_g1;
    uint64_t *a_query, *b_g1_query, *b_g2_query, *h_query, *l_query;
} mg_pk_out;
int mg_groth16_setup(mg_curve_t curve, const mg_csr *a, const mg_csr *b, const mg_csr *c, uint64_t num_constraints,
                     uint64_t n_vars, uint64_t n_inputs, const uint64_t *toxic_mont /* 5 x 4: alpha beta gamma delta tau */,
                     const uint64_t *g1_generator, const uint64_t *g2_generator, const mg_pk_out *out);

/* ---- phase-2 key initialisation of the trusted setup: `mpc::initialize` (manta-trusted-setup/src/groth16/mpc.rs:353-431),
 *      which `groth16_phase2_prepare` runs once per circuit on a powers-of-tau accumulator. Synchronous; all device work on
 *      the calling thread's setup stream. --------------------------------------------------------------------------- */
/* out[j] = sum over terms t and stored entries (i, j) of M_t of [M_t[i][j]] * bases[t][i]  (n_cols affine points).
 * Parity-test surface of mg_mpc_initialize and a primitive of its own (`specialize_to_phase_2`, mpc.rs:251-294).
 * bases_affine[t]: m affine Montgomery points (zeros = infinity, honoured); mats[t]: m rows, n_cols columns, Montgomery
 * coefficients (the multiplier is `coeff.into_repr()`; a stored zero contributes nothing, repeated (row, column) entries
 * each count). group: 1 or 2. entries_per_lane: sorted entries per lane of the segmented sum, 0 = the library's choice;
 * no result depends on it. One sort, one multiplication kernel, one segmented sum and its merge levels, one batched
 * normalisation for the whole call: the number of launches and copies does not depend on n_cols.
 * MG_ERROR_INVALID_ARGUMENT before any device work, with out_affine untouched: n_terms = 0, m = 0, n_cols = 0, a NULL
 * basis or matrix, a row_ptr that does not rise from 0 to nnz, a column >= n_cols, 2^31 stored entries or more in all, more columns than the
 * 32-bit word index of the sums holds (2^32 / words of an XYZZ point: 119 M for BN254 G1, 38 M for BLS12-381 G2). */
int mg_qap_columns(mg_curve_t curve, int group, size_t n_terms, const uint64_t *const *bases_affine,
                   const mg_csr *const *mats, uint64_t m, uint64_t n_cols, uint32_t entries_per_lane,
                   uint64_t *out_affine);

typedef struct {
    uint64_t n_g1, n_g2; /* tau_powers_g1[n_g1]; tau_powers_g2, alpha_tau_powers_g1, beta_tau_powers_g1: [n_g2] */
    const uint64_t *tau_powers_g1, *tau_powers_g2, *alpha_tau_powers_g1, *beta_tau_powers_g1, *beta_g2;
} mg_kzg_view;

/* `mpc::initialize` (mpc.rs:353-431) after synthesis: the phase-2 key of a circuit from a KZG accumulator,
 * gamma = delta = 1. Output arrays as for mg_groth16_setup, h_query[h_len].
 * D = next_pow2(num_constraints + n_inputs); beyond the field's two-adicity: MG_ERROR_DOMAIN_TOO_LARGE (the reference's
 * `TooManyConstraints`; decided before the matrices are read). h_len = D - 1 (what ark-groth16 keys carry) or D (what the reference's loop :372-377 produces).
 * h_query[i] = tau^(i+D) G - tau^i G; four inverse group NTTs of the first D powers; `add_dummy_constraints` (:299-312);
 * a_query = A^T tauL, b_g1_query = B^T tauL, b_g2_query = B^T tauL2, ext = A^T betaL + B^T alphaL + C^T tauL,
 * gamma_abc_g1 = ext[..n_inputs], l_query = ext[n_inputs..]; alpha_g1, beta_g1, beta_g2 from the accumulator; delta_g1,
 * gamma_g2, delta_g2 = the generators passed in. Each power vector is uploaded once, the Lagrange bases stay in device
 * memory between the NTTs and the column sums, only the key comes back.
 * MG_ERROR_INVALID_ARGUMENT before anything is allocated, with `out` untouched (as after every failure): a NULL argument,
 * n_inputs = 0 or >= n_vars, a malformed matrix (as for mg_ctx_set_r1cs), another h_len, n_g1 < D + h_len, n_g2 < D, a
 * domain above 2^26 that the field would still allow (the group NTT's own limit, as for mg_group_ntt), 2^31 column-sum
 * entries (2 nnz(A) + 2 nnz(B) + nnz(C) + 2 n_inputs) or more, more columns (3 n_vars) than the 32-bit word index of the sums
 * holds (about 39 M variables on BN254, 25 M on BLS12-381). */
int mg_mpc_initialize(mg_curve_t curve, const mg_kzg_view *powers, const mg_csr *a, const mg_csr *b, const mg_csr *c,
                      uint64_t num_constraints, uint64_t n_vars, uint64_t n_inputs, uint64_t h_len,
                      const uint64_t *g1_generator, const uint64_t *g2_generator, const mg_pk_out *out);

/* Uploads and re-lays the proving key once (lifetime = the Rust ProvingContext). */
int mg_ctx_create(mg_curve_t curve, const mg_pk_view *pk, mg_ctx **out);
/* The same with everything a deployment decides per context in ONE struct (the entry points below are shorthands for it):
 * a signer holds three contexts at once -- `MultiProvingContext { to_private, private_transfer, to_public }`,
 * manta-accounting/src/transfer/canonical.rs:561-588 -- so what a context may spend on speed is a property of the context,
 * not of the process.
 *   struct_size       sizeof(mg_ctx_opts), written by mg_ctx_opts_init: the struct can grow without breaking callers
 *   exchange          how the partial points of a context sharded over `devices` meet: MG_EXCHANGE_HOST -- through pinned host
 *                     memory, summed on the host -- or MG_EXCHANGE_RCCL -- every device folds its five partial points per proof
 *                     on the GPU, one grouped ncclAllGather of 5 x 256 B (BN254) per device and proof over xGMI inside the
 *                     library (ncclCommInitAll over the list: no duplicate devices), assembly as in mg_groth16_assemble.
 *                     BASELINE north_star: "final RCCL reduce of partial EC points over xGMI" behind the C ABI; caller
 *                     manta-accounting/src/transfer/mod.rs:695-715. librccl.so is loaded when first asked for; if it is
 *                     missing the call fails with MG_ERROR_STATE (no silent fallback).
 *   full_table_bytes  HBM this context may spend on FULL tables of its five queries together (single proofs run on them:
 *                     no sort, no bucket reduce on their latency chain), per device: the widest windows that fit are chosen,
 *                     0 = none (bucket tables only), negative = the default, a tenth of the device's HBM (28.8 GB on an
 *                     MI355X: three contexts use 30 %). Never more than 40 % of what is free at creation. Negative: the tuning's
 *                     full_table_bytes applies (where MANTA_FULL_TABLE_GB lands), else the default.
 *   devices/n_devices range-shard every MSM over these devices inside this process (mg_ctx_create_sharded)
 *   shard/n_shards    this process holds one slice (mg_ctx_create_shard); n_shards <= 1: the whole key
 *   task_mask         mg_ctx_create_task; 0 or 0x1f: all five MSMs
 * At most one of the three placements may be used. */
#define MG_EXCHANGE_HOST 0u
#define MG_EXCHANGE_RCCL 1u
/* ---- tuning: everything a DEPLOYMENT decides about how the library schedules its work, as one struct (none of it changes a
 *      result -- tests/test_gpu_profiles.py proves every field and every environment name below leaves proof bytes unchanged).
 *      Reference counterpart: `ProvingContext` carries no tuning at all (manta-crypto/src/arkworks/groth16.rs:216-245): the
 *      arkworks prover has one schedule; this struct is what the GPU path adds next to it. A Rust host fills it once
 *      (rust/mantagpu-sys mirrors it) instead of exporting environment variables. Process-wide values: mg_get_tuning /
 *      mg_set_tuning (contexts copy them when they are created); per context: mg_ctx_opts.tuning.
 *      The shipped library reads the environment in ONE place, once, as the initial process-wide values -- the 14 variables of
 *      mg_tuning_env_names() (plus MANTA_RCCL_LIB, the path of librccl.so): MANTA_GRAPH (single | split | off),
 *      MANTA_GRAPH_BATCH, MANTA_PROVE_STREAMS, MANTA_Z3_LINEAR, MANTA_COALESCE, MANTA_COALESCE_GATHER_US, MANTA_BATCH_INFLIGHT,
 *      MANTA_QUEUE_AWARE, MANTA_MSM_DEDICATED_QUEUES, MANTA_PROVE_C / _CW / _CH / _CG2, MANTA_FULL_TABLE_GB. Every other knob of
 *      the measurement campaigns is compiled in at its measured optimum (a unit rebuilt with -DMG_DIAG reads it again).
 *      A variable applies only if its WHOLE string parses as the field's kind (a decimal integer that fits 32 bits; off | single |
 *      split | 0 | 1 | 2 for a graph mode; a finite number of GB whose byte count fits 64 bits, negative = -1) and the field's
 *      range accepts the value; anything else is ignored and the default stays.
 *   struct_size           sizeof(mg_tuning), written by mg_tuning_init / mg_get_tuning
 *   graph_mode            replay of a pass's GPU side as hipGraphs: 1 = two graphs per pass (default), 2 = six single-stream graphs,
 *                         0 = eager launches
 *   graph_mode_batch      the same for passes of >= 4 proofs; -1 = as graph_mode
 *   prove_streams         streams of a forked pass: 3, 4, 5 or 6 (default)
 *   linear_chains         single proofs as three linear graphs on three hardware queues: 0 never, 1 a lone proof only, 2 also
 *                         beside other passes, 3 (default) the same with the yielding chain chosen by what the proof runs beside
 *   coalesce_inflight     passes of coalesced concurrent mg_groth16_prove calls on the GPU: 0 = no coalescing, default 2, <= 4
 *   coalesce_gather_us    how long the leader of such a pass waits for the callers of the pass that has just ended (default 100)
 *   batch_inflight        passes of one mg_groth16_prove_batch call in flight (default 3)
 *   queue_aware           1 (default): single-proof slots get streams on measured hardware queues; 0: plain pooled streams.
 *                         Per context: a context follows its own value, whatever the process-wide one is
 *   msm_dedicated_queues  a stand-alone MSM (mg_msm_launch) on a stream with a hardware queue of its own: its pipelined rate then no
 *                         longer depends on the streams the rest of the process created (390-398 Mscalar/s at 2^20 for every
 *                         creation order against 317-394). 1 (default) = only while NO proving / verifying context is alive in
 *                         the process (beside proof passes the dedicated queues cost far more than they give), 2 = always,
 *                         0 = never. Such streams are BLOCKING streams: they order themselves against the host's NULL-stream work
 *                         (the library itself puts nothing on the NULL stream). Process-wide by nature: a stand-alone MSM has
 *                         no context, so the value in mg_ctx_opts.tuning is not consulted
 *   window_bits_*         window widths of a context's key tables, 0 = the library's choice: narrow = the latency tables of
 *                         a / b_g1 / l (setting it forces ONE width for every bucket table and leaves the full and wide tables
 *                         out), wide = the batched-pass tables, h = the h query, g2 = b_g2
 *   full_table_bytes      default HBM budget of a context's full tables (mg_ctx_opts.full_table_bytes >= 0 takes precedence);
 *                         -1 = a tenth of the device's HBM, 0 = none */
typedef struct mg_tuning {
    uint32_t struct_size;
    int32_t graph_mode;
    int32_t graph_mode_batch;
    int32_t prove_streams;
    int32_t linear_chains;
    int32_t coalesce_inflight;
    int32_t coalesce_gather_us;
    int32_t batch_inflight;
    int32_t queue_aware;
    int32_t msm_dedicated_queues;
    int32_t window_bits_narrow;
    int32_t window_bits_wide;
    int32_t window_bits_h;
    int32_t window_bits_g2;
    int64_t full_table_bytes;
} mg_tuning;
int mg_tuning_init(mg_tuning *t);      /* the compiled-in defaults (no environment) */
int mg_get_tuning(mg_tuning *t);       /* the process-wide values in force */
int mg_set_tuning(const mg_tuning *t); /* validated as a whole (MG_ERROR_INVALID_ARGUMENT leaves everything as it was); contexts
                                          created afterwards use it, the environment no longer applies */
/* NULL-terminated list of the environment variables the shipped library reads (the tuning table + MANTA_RCCL_LIB) */
const char *const *mg_tuning_env_names(void);

typedef struct mg_ctx_opts {
    uint32_t struct_size;
    uint32_t exchange;
    int64_t full_table_bytes;
    const int *devices;
    int32_t n_devices;
    int32_t shard, n_shards;
    uint32_t task_mask;
    const mg_tuning *tuning; /* this context's tuning (read during the call); NULL = the process-wide values */
} mg_ctx_opts;
int mg_ctx_opts_init(mg_ctx_opts *opts); /* defaults: host exchange, default table budget, current device, whole key */
int mg_ctx_create_ex(mg_curve_t curve, const mg_pk_view *pk, const mg_ctx_opts *opts /* NULL = defaults */, mg_ctx **out);
/* ... and from the key's wire format (mg_ctx_create_from_bytes below), checksum32 = the expected BLAKE3 digest or NULL:
 * the integrity check of mg_ctx_create_from_bytes_checked in front of EVERY placement. */
int mg_ctx_create_from_bytes_ex(mg_curve_t curve, const uint8_t *bytes, size_t len, const uint8_t *checksum32,
                                const mg_ctx_opts *opts, mg_ctx **out);
/* The proving key range-sharded over a list of devices (BASELINE configs[3]: "PrivateTransfer full proof, MSM
 * sharded across 8 GPUs"): device g holds the g-th contiguous slice of every query with its window tables. A proof
 * uploads the assignment to every device, each recomputes the witness map (cheaper than broadcasting h, SURVEY.md
 * 8(e)) and runs its five partial MSMs; the 5 x G partial points are added on the host by the same code that folds
 * the single-GPU results. Proof bytes are identical to the single-device context's. devices may repeat. */
int mg_ctx_create_sharded(mg_curve_t curve, const mg_pk_view *pk, const int *devices, int n_devices, mg_ctx **out);
int mg_ctx_create_from_bytes_sharded(mg_curve_t curve, const uint8_t *bytes, size_t len, const int *devices,
                                     int n_devices, mg_ctx **out);
/* One process per GPU (what `python -m torch.distributed.run` starts; BASELINE configs[3] "MSM sharded across 8 x MI355X via
 * RCCL/xGMI"; caller: manta-accounting/src/transfer/mod.rs:695-715 -> groth16.rs:589-600): THIS process holds shard
 * `shard` of `n_shards` -- the same contiguous slices mg_ctx_create_sharded gives device g -- on the current device.
 *   mg_groth16_partials_launch: uploads z (every rank has the whole assignment and recomputes the witness map), runs the five
 *     MSMs over this shard's slices and leaves, per proof, the five partial results a | b_g1 | b_g2 | l | h folded on the
 *     device in slots of mg_partials_slot_limbs() u64 (XYZZ points as in mg_msm_result_to_device, G1 ones padded) at
 *     d_out[k][5][slot]; `stream` (hipStream_t, e.g. the stream RCCL runs on) waits for them. k <= 32. No host sync.
 *   mg_groth16_partials_finish: returns the pass's slot once the consumer has read d_out.
 *   mg_groth16_assemble: parts = n_parts gathered copies of [k][5][slot] in HOST memory (one fused all_gather of <= 1.9 KB
 *     per rank and proof); adds them and finishes the proofs exactly like mg_groth16_prove -- bytes identical to the
 *     single-GPU context's. Host-only work: any rank (or all) may call it. */
/* A shard context with n_shards > 1 holds ONE slice of every query: mg_groth16_prove / mg_groth16_prove_batch on it return
 * MG_ERROR_STATE (a proof built from one slice's MSMs would be silently invalid); only the partials interface and
 * mg_witness_map work on it. */
int mg_ctx_create_shard(mg_curve_t curve, const mg_pk_view *pk, int shard, int n_shards, mg_ctx **out);
/* The alternative placement of SURVEY.md 8(e): TASK-parallel -- this process holds the whole key and computes the MSMs of
 * task_mask in full (bit 0 a, 1 b_g1, 2 b_g2, 3 l, 4 h; the witness map only when it owns h); for the others
 * mg_groth16_partials_launch writes the point at infinity, so the same gather + mg_groth16_assemble finish the proof. Five point
 * transfers instead of a sum over ranks, at most five busy GPUs. mg_groth16_prove on such a context returns MG_ERROR_STATE. */
#define MG_TASK_A 1u
#define MG_TASK_B_G1 2u
#define MG_TASK_B_G2 4u
#define MG_TASK_L 8u
#define MG_TASK_H 16u
int mg_ctx_create_task(mg_curve_t curve, const mg_pk_view *pk, unsigned task_mask, mg_ctx **out);
typedef struct mg_partials_job mg_partials_job;
size_t mg_partials_slot_limbs(const mg_ctx *ctx);
int mg_groth16_partials_launch(const mg_ctx *ctx, uint64_t k, const uint64_t *z_mont, uint64_t *d_out, void *stream,
                               mg_partials_job **job);
int mg_groth16_partials_finish(mg_partials_job *job);
int mg_groth16_assemble(const mg_ctx *ctx, uint64_t k, int n_parts, const uint64_t *parts, const uint64_t *r_mont,
                        const uint64_t *s_mont, uint8_t *proofs_out);
/* Same, from the key's wire format: arkworks 0.3 `ProvingKey::serialize_unchecked` bytes (uncompressed points,
 * no curve checks) exactly as `ProvingContext::decode` reads them (manta-crypto/src/arkworks/groth16.rs:268-288)
 * and `generate_parameters` / manta-parameters ship them (data/pay/proving/ *.lfs). */
int mg_ctx_create_from_bytes(mg_curve_t curve, const uint8_t *bytes, size_t len, mg_ctx **out);
/* The same behind manta-parameters' integrity check: `manta_parameters::verify(data, checksum)` = `blake3::hash(data) ==
 * checksum` (manta-parameters/src/lib.rs:173-177; `Get::get` refuses a file whose digest differs from data.checkfile,
 * lib.rs:150-170). checksum = the 32-byte BLAKE3 digest the caller expects (`HasChecksum::CHECKSUM`); a mismatch returns
 * MG_ERROR_CHECKSUM and nothing is uploaded. mg_blake3 is the digest itself (host code, any length). */
int mg_ctx_create_from_bytes_checked(mg_curve_t curve, const uint8_t *bytes, size_t len, const uint8_t checksum[32],
                                     mg_ctx **out);
int mg_blake3(const uint8_t *data, size_t len, uint8_t out32[32]);
/* Blake2s-256 (RFC 7693; unkeyed, no salt, no personalisation -- the reference's `Blake2s256::new()`): host code, any length,
 * compiled from the same source as the hash of the signature kernels below. */
int mg_blake2s256(const uint8_t *data, size_t len, uint8_t out32[32]);
/* The same hash with a digest of out_len bytes, 1..32 (`Blake2sVar::new(out_len)`; the length is part of the parameter word, so
 * this is no prefix of the 32-byte digest; out_len = 32 is mg_blake2s256), and AES-256-GCM with a 12-byte nonce, no associated
 * data and a 16-byte tag (the `aes-gcm` crate's `Aead`): host code, any length, compiled from the same sources as the note
 * kernels at the end of this header. decrypt = 0: `in` is len bytes of plaintext, `out` gets len + 16 (ciphertext | tag).
 * decrypt != 0: `in` is ciphertext | tag (len >= 16), `out` gets len - 16 bytes, *ok = the tag verified; where it did not, the
 * output is zeros. `ok` may be NULL when encrypting. */
int mg_blake2s(const uint8_t *data, size_t len, size_t out_len, uint8_t *out);
int mg_aes256_gcm(const uint8_t key[32], const uint8_t nonce[12], const uint8_t *in, size_t len, int decrypt, uint8_t *out,
                  int *ok);
/* Once per circuit shape: the matrices of `cs.to_matrices()` (identical for every proof of a shape). Validated
 * in full before anything changes (row_ptr monotone from 0 to nnz, column indices < V); a rejected call leaves
 * the context as it was. */
int mg_ctx_set_r1cs(mg_ctx *ctx, const mg_csr *a, const mg_csr *b, const mg_csr *c, uint64_t num_constraints);
/* One proof. z = instance || witness (V x 4 u64 Montgomery), r, s = the two blinding scalars drawn by
 * the shim with the reference's own RNG in create_random_proof's order (Montgomery).
 * proof_out: 128 B (BN254) / 192 B (BLS12-381). Re-entrant on one context: calls that arrive while two passes are on
 * the GPU are grouped into ONE batched pass by the next caller (the reference's simulation drives a context from six
 * threads, manta-pay/src/bin/simulation.rs:36-38); the bytes of a proof do not depend on the grouping. */
int mg_groth16_prove(const mg_ctx *ctx, const uint64_t *z_mont, const uint64_t r_mont[4], const uint64_t s_mont[4],
                     uint8_t *proof_out);
/* k proofs of the context's circuit (throughput mode: a wallet / ledger simulation proving many transfers
 * against one ProvingContext, manta-pay/src/simulation/mod.rs:75-79; the shim collects k `prove` calls or
 * exposes a `prove_many`). Up to 32 proofs are ONE pass of the GPU pipeline; a longer batch is streamed
 * through as passes of 32 with three in flight (library threads), so one call with k >= 96 keeps the
 * GPU as busy as three callers would. z = k assignments back to back (k x V x 4 u64), r, s = k blinding
 * scalars each (k x 4 u64), proofs_out = k proofs back to back. Proof q is byte-identical to
 * mg_groth16_prove(ctx, z_q, r_q, s_q). 1 <= k <= 1024. */
int mg_groth16_prove_batch(const mg_ctx *ctx, uint64_t k, const uint64_t *z_mont, const uint64_t *r_mont,
                           const uint64_t *s_mont, uint8_t *proofs_out);
/* h = R1CStoQAP::witness_map(z): D x 4 u64 Montgomery coefficients (tests / parity) */
int mg_witness_map(const mg_ctx *ctx, const uint64_t *z_mont, uint64_t *h_out_mont);
/* `R1CS::is_satisfied` (manta-crypto/src/constraint.rs:30,41; manta-crypto/src/arkworks/constraint/mod.rs:130-132 -> ark-relations
 * ConstraintSystem::is_satisfied / which_is_unsatisfied) for k assignments at once, on the GPU: first_unsatisfied[j] = the lowest
 * row i < num_constraints of assignment j with <A_i, z> <B_i, z> != <C_i, z>, or MG_R1CS_SATISFIED; n_unsatisfied[j] (the array
 * may be NULL) = the number of such rows. Only the constraint rows are looked at, as in ark-relations: not the prover's
 * input-consistency rows, not z_0. z = k assignments back to back (k x V x 4 u64 Montgomery, every element below the modulus: as
 * for mg_groth16_prove a larger one is the caller's error and its verdict unspecified -- memory stays safe). mg_groth16_prove
 * turns an unsatisfied assignment into a non-verifying proof with status 0, as ark-groth16 does in release builds; these calls
 * restore what its debug_assert! would have said, per assignment and with the row.
 * mg_ctx_r1cs_check: against the matrices resident in the context (MG_ERROR_STATE before mg_ctx_set_r1cs); safe beside proofs in
 * flight on the same context. mg_r1cs_check: no proving key needed -- the reference's R1CS::is_satisfied has none either; the
 * matrices (checked like mg_ctx_set_r1cs's, against n_vars columns) are uploaded for the call.
 * MG_ERROR_INVALID_ARGUMENT before any device work, the outputs untouched: a NULL context, z or first_unsatisfied with k > 0, a
 * malformed matrix, n_vars = 0, an unknown curve. k = 0 succeeds and num_constraints = 0 reports every assignment satisfied,
 * both without device work. */
#define MG_R1CS_SATISFIED UINT64_MAX
int mg_ctx_r1cs_check(const mg_ctx *ctx, uint64_t k, const uint64_t *z_mont, uint64_t *first_unsatisfied,
                      uint64_t *n_unsatisfied);
int mg_r1cs_check(mg_curve_t curve, const mg_csr *a, const mg_csr *b, const mg_csr *c, uint64_t num_constraints,
                  uint64_t n_vars, uint64_t k, const uint64_t *z_mont, uint64_t *first_unsatisfied, uint64_t *n_unsatisfied);
uint64_t mg_ctx_domain_size(const mg_ctx *ctx);
/* HBM held by the context's key tables, bytes: out[0] = bucket tables (2^(c*w)*P per window, two widths), out[1] = FULL tables
 * (every multiple of every window; single proofs run on them; mg_ctx_opts.full_table_bytes bounds them, 0 = none). The h
 * tables exist once mg_ctx_set_r1cs has run. Summed over the devices of a sharded context. */
int mg_ctx_table_bytes(const mg_ctx *ctx, uint64_t out2[2]);
uint64_t mg_ctx_num_variables(const mg_ctx *ctx); /* V: the length every assignment must have */
uint64_t mg_ctx_num_inputs(const mg_ctx *ctx);    /* P */
int mg_ctx_num_shards(const mg_ctx *ctx);
void mg_ctx_destroy(mg_ctx *ctx);

/* ---- verification: replaces `Groth16::verify` (manta-crypto/src/arkworks/groth16.rs:603-609 -> ark-groth16 0.3
 *      verify_with_processed_vk) and `VerifyingContext` with its codec (groth16.rs:305-539) -------------------------- */
typedef struct mg_vk mg_vk; /* device-resident PreparedVerifyingKey */
/* `VerifyingContext::new(&vk)` = ArkGroth16::process_vk (groth16.rs:323-327): from the key's five components (affine
 * Montgomery; gamma_abc_g1 = n_inputs points incl. the one for the constant input) everything the prepared key holds is
 * computed on the GPU -- the G2Prepared line coefficients of -gamma_g2 and -delta_g2 and e(alpha_g1, beta_g2) with
 * arkworks' final exponentiation. */
int mg_vk_create(mg_curve_t curve, const uint64_t *alpha_g1, const uint64_t *beta_g2, const uint64_t *gamma_g2,
                 const uint64_t *delta_g2, const uint64_t *gamma_abc_g1, uint64_t n_inputs, mg_vk **out);
/* `impl Decode for VerifyingContext` (groth16.rs:498-517): the wire format of manta-parameters' verifying-key files
 * (vk compressed | e(alpha, beta) | two G2Prepared). Checked like `CanonicalDeserialize::deserialize`: canonical field
 * encodings, points on the curve and in the prime-order subgroup, no trailing bytes. */
int mg_vk_create_from_bytes(mg_curve_t curve, const uint8_t *bytes, size_t len, mg_vk **out);
/* `impl Encode for VerifyingContext` (groth16.rs:519-533): byte-identical to the reference's file for the same key. */
size_t mg_vk_encoded_size(const mg_vk *vk);
int mg_vk_encode(const mg_vk *vk, uint8_t *out);
int mg_vk_alpha_beta(const mg_vk *vk, uint8_t *out /* 12 Fq elements, 384 / 576 B */);
uint64_t mg_vk_num_inputs(const mg_vk *vk);
void mg_vk_destroy(mg_vk *vk);
/* One proof. inputs = the n_inputs - 1 public inputs (Montgomery Fr, `Input = Vec<E::Fr>`), proof_points = a | b | c
 * affine Montgomery (the in-memory ark_groth16::Proof<E>; mg_proof_decode gives it from the 128 / 192 proof bytes).
 * *ok = 1 iff the proof verifies; the return value reports only operational failures. */
int mg_groth16_verify(const mg_vk *vk, const uint64_t *inputs_mont, const uint64_t *proof_points, int *ok);
/* k proofs against one key by random linear combination: rand128 = k x 2 u64 -- 128 random bits per proof from the
 * caller's RNG, not both words zero. Proof i enters with the coefficient k1 + lambda k2, (k1, k2) its two words and
 * lambda the eigenvalue of G1's endomorphism (x, y) -> (beta x, y): 2^128 - 1 distinct non-zero values, and k_i A_i
 * then costs 64 doublings instead of 128. k + 3 Miller loops (two wavefronts each), k scalar multiplications, two small
 * MSMs and one final exponentiation. *ok = 1 iff ALL k proofs verify (up to the 2^-128 soundness error of the
 * combination); on 0 call mg_groth16_verify_each on the same rows to find the offenders: one pass over the block, not k
 * single verifications. */
int mg_groth16_verify_batch(const mg_vk *vk, uint64_t k, const uint64_t *inputs_mont, const uint64_t *proof_points,
                            const uint64_t *rand128, int *ok);
/* ---- a verdict per item: many small independent pairing products in one pass. The pairs of MG_VERIFY_EACH_CHUNK groups
 *      go through ONE Miller-loop launch (two wavefronts per pair) and ONE launch of a wavefront per group that multiplies
 *      the group's Miller values, runs the final exponentiation and compares on the device; only the verdict bytes come
 *      back. Larger calls run chunk after chunk, so device and pinned memory of a call do not depend on the count: per
 *      pair 0.7 KB (BN254) / 1.1 KB (BLS12-381) of pooled workspace (G1, G2, coefficient pointer, flag, the Miller value
 *      and its share of a scratch array), i.e. at most 2.8 / 4.1 MB for the three pairs of a proof and 59 / 88 MB at the
 *      largest group size, the pool's growth margin of a quarter included; plus for mg_groth16_verify_each the pooled workspace of one MSM of
 *      MG_VERIFY_EACH_CHUNK x n_inputs scalars. Synchronous, thread-safe, re-entrant; pooled workspaces and streams only
 *      (no allocation per call once the pool is warm, nothing on the NULL stream). The time does not depend on the
 *      verdicts, and the return value reports operational failures only. */
#define MG_VERIFY_EACH_CHUNK 1024u
/* n_groups independent mg_pairing_check's of group_size pairs each: ok[t] = 1 iff prod_j e(P[t][j], Q[t][j]) == 1.
 * g1_affine / g2_affine: [n_groups][group_size] points, group-major as a caller holds them. n_groups = 0 succeeds and
 * writes nothing; group_size = 0 or above 64, or a NULL array with n_groups > 0: MG_ERROR_INVALID_ARGUMENT. */
int mg_pairing_check_each(mg_curve_t curve, const uint64_t *g1_affine, const uint64_t *g2_affine, size_t group_size,
                          size_t n_groups, uint8_t *ok);
/* k proofs against one key, a verdict each: ok[i] is exactly what mg_groth16_verify would answer for row i (rows with
 * points at infinity included). inputs_mont and proof_points as for mg_groth16_verify_batch. The prepared inputs of a chunk
 * are one batched MSM over the key's tables, folded on the device and read there by the Miller loops. Where an MSM launch
 * takes fewer scalar vectors than the chunk (65 535 vectors, 2^31 digit pairs, a key space of 2^24) the chunk shrinks to
 * that. k = 0 succeeds and writes nothing; k above 2^20, a NULL array, or inputs_mont = NULL with n_inputs > 1:
 * MG_ERROR_INVALID_ARGUMENT before any device work. */
int mg_groth16_verify_each(const mg_vk *vk, uint64_t k, const uint64_t *inputs_mont, const uint64_t *proof_points,
                           uint8_t *ok);
/* prod_i e(P_i, Q_i) == 1 ? -- the pairing-product test behind `PairingEngineExt::has_same` / `same_ratio`
 * (manta-crypto/src/arkworks/pairing.rs:88-109), which the trusted-setup verifier applies to random linear
 * combinations of whole queries (`verify_transform`, manta-trusted-setup/src/groth16/mpc.rs:470-508). P_i affine
 * G1, Q_i affine G2 (Montgomery limbs; an all-zero point is infinity and its pair contributes 1). n Miller loops
 * (one wavefront each, every Q_i prepared alongside by a second one) and one final exponentiation. */
int mg_pairing_check(mg_curve_t curve, const uint64_t *g1_affine, const uint64_t *g2_affine, size_t n, int *ok);
/* The pairing's building blocks, each alone over host arrays: a parity-test surface for the device functions every
 * pairing runs (as mg_field_op and mg_fpr_raw_op are for the fields), not needed by the shim. Synchronous, one launch on
 * the calling thread's setup stream. All values are Montgomery words (uint32), canonical (below q); an Fq12 is twelve Fq
 * in arkworks' memory order (slot 3 i + j = the coefficient of w^(i + 2 j), each c0 then c1), as mg_vk_alpha_beta's
 * value before serialisation.
 *   Fq12 operations, one element per single-wavefront workgroup, a and out [n][12 Fq]:
 *     MUL12 a b (b [n][12 Fq])   SQR12 a^2   CYC_SQR12 a^2 for a in the cyclotomic subgroup
 *     ELL a times the line b = [n][3 Fq2], coefficient t at w^t (BN254: w^0, w^1, w^3; BLS12-381: w^0, w^2, w^3) -- the
 *         Miller loop's line product with the coefficients as they come out of their scaling by the G1 point
 *     FROB12_k a^(q^k)   CONJ12 a^(q^6)   INV12 1/a (a != 0)
 *     EXP_BY_X a^x for a in the cyclotomic subgroup, x the curve's signed parameter   FINAL_EXP arkworks' final_exponentiation
 *   Fq and Fq2 helpers, one element per lane:
 *     FQ_INV_EUCLID 1/a (a, out [n][Fq], a != 0)   FQ_HALF a/2   FQ2_MUL a b (a, b, out [n][Fq2])   FQ2_MUL_XI xi a
 *     FQ_LINCOMB sum_m coeffs[i][m] a[i][m]: a [n][10][Fq], coeffs [n][10] in -255..255, out [n][Fq] -- one `lincomb` of
 *         ten operands as the second stage of the squarings and the line product calls it
 * MG_ERROR_INVALID_ARGUMENT before any device work: an unknown curve or op, a missing operand, n = 0 or above
 * MG_PAIRING_OP_MAX, a row of coefficients whose positive or negative sum reaches 256. */
#define MG_PAIRING_MUL12 0
#define MG_PAIRING_SQR12 1
#define MG_PAIRING_CYC_SQR12 2
#define MG_PAIRING_ELL 3
#define MG_PAIRING_FROB12_1 4
#define MG_PAIRING_FROB12_2 5
#define MG_PAIRING_FROB12_3 6
#define MG_PAIRING_CONJ12 7
#define MG_PAIRING_INV12 8
#define MG_PAIRING_EXP_BY_X 9
#define MG_PAIRING_FINAL_EXP 10
#define MG_PAIRING_FQ_INV_EUCLID 11
#define MG_PAIRING_FQ_HALF 12
#define MG_PAIRING_FQ2_MUL 13
#define MG_PAIRING_FQ2_MUL_XI 14
#define MG_PAIRING_FQ_LINCOMB 15
#define MG_PAIRING_LINCOMB_OPERANDS 10
#define MG_PAIRING_OP_MAX 65536
int mg_pairing_op(mg_curve_t curve, int op, const uint32_t *a, const uint32_t *b, const int16_t *coeffs, size_t n,
                  uint32_t *out);
/* `Proof::deserialize` (arkworks compressed a | b | c) -> a | b | c affine Montgomery limbs; rejects non-canonical
 * encodings, points off the curve or outside the subgroup. */
int mg_proof_decode(mg_curve_t curve, const uint8_t *proof_bytes, uint64_t *points_out);

/* ---- batched point codec: arkworks 0.3 short-Weierstrass encodings on the GPU, one point per lane. Replaces per-point
 *      `GroupAffine: CanonicalDeserialize` + `is_in_correct_subgroup_assuming_on_curve` (ark-ec 0.3) as run by
 *      `Proof::deserialize`, `kzg::Accumulator`'s deserializer (manta-trusted-setup/src/groth16/kzg.rs:607-690, `C::check`
 *      on every power) and `mpc::State::check` (groth16/mpc.rs:79-100), and `CanonicalSerialize` of the same points.
 *      Encoding: x (G2: x.c0 || x.c1) little-endian canonical, flags in the two top bits of the LAST byte of the record
 *      (bit 6 = infinity, bit 7 = y is the lexicographically larger root, c1 first then c0; both set is invalid);
 *      uncompressed = x || y with the flags on y. Every coordinate read must be canonical, infinity's included. The
 *      subgroup test is [r]P == O. Synchronous, thread-safe, on the calling thread's setup stream; the points go through
 *      the GPU 65 536 at a time (device memory and pinned staging of a call < 26 MB whatever n); n = 0 succeeds. The return
 *      value reports only operational failures: bad points are reported per point. ------------------------------------ */
#define MG_POINT_OK 0
#define MG_POINT_BAD_ENCODING 1    /* coordinate >= q, both flag bits set, or a bit above the modulus set */
#define MG_POINT_NOT_ON_CURVE 2    /* uncompressed: y^2 != x^3 + b; compressed: x^3 + b has no square root */
#define MG_POINT_NOT_IN_SUBGROUP 3 /* on the curve, [r]P != O */
/* n encodings of 32/48 (G1) or 64/96 (G2) bytes each, doubled when uncompressed -> n affine Montgomery points (zeros for
 * infinity and for every rejected point) and status[i] = MG_POINT_*; status and n_bad (rejected count) may be NULL.
 * checked = 1: `CanonicalDeserialize::deserialize` (curve and subgroup); checked = 0: `deserialize_unchecked`, only for
 * uncompressed input (as the proving-key reader): canonical coordinates and flags only. */
int mg_points_decode(mg_curve_t curve, int group, const uint8_t *bytes, size_t n, int compressed, int checked,
                     uint64_t *out_affine_mont, uint8_t *status, size_t *n_bad);
/* `C::check` / `State::check` on n affine Montgomery points in memory (zeros = infinity): MG_POINT_BAD_ENCODING for a
 * coordinate >= q, else curve, then subgroup. status must hold n bytes; n_bad may be NULL. */
int mg_points_check(mg_curve_t curve, int group, const uint64_t *affine_mont, size_t n, uint8_t *status, size_t *n_bad);
/* `CanonicalSerialize` of n affine Montgomery points, byte for byte mg_point_serialize, back to back into out. */
int mg_points_encode(mg_curve_t curve, int group, const uint64_t *affine_mont, size_t n, int compressed, uint8_t *out);
/* k compressed proofs a | b | c back to back (128 / 192 bytes each) -> k rows a | b | c of affine Montgomery limbs, as
 * mg_proof_decode gives one: ok[i] = 1 iff that call would accept proof i; a rejected proof's row is zeros. Then
 * mg_groth16_verify_batch on the accepted rows. */
int mg_proofs_decode(mg_curve_t curve, const uint8_t *proof_bytes, size_t k, uint64_t *points_out, uint8_t *ok);

/* ---- the same codec for the point records of Perpetual Powers of Tau challenge / response files (`PpotSerializer`,
 *      manta-trusted-setup/src/groth16/ppot/serialization.rs:52-379; per point on the host there: `read_g1_powers`,
 *      `read_g2_powers`, `curve_point_checks`). Bn254 only -- the ceremony's curve; any other curve is
 *      MG_ERROR_INVALID_ARGUMENT. A record is the concatenation of 32-byte BIG-endian base-field elements: G1 x | y (64 B),
 *      compressed x (32 B); G2 x.c1 | x.c0 | y.c1 | y.c0 (128 B), compressed x.c1 | x.c0 (64 B). Bits 7 and 6 of byte 0 are
 *      flags, cleared from the first element only: bit 6 = infinity (every other bit of the record must then be zero);
 *      bit 7 = y is the greater of y, -y in a compressed record (arkworks order, c1 first), and "compressed" -- an error -- in
 *      an uncompressed one. Coordinates are read mod q (`from_be_bytes_mod_order`): a value >= q is reduced, not rejected.
 *      Same kernels, chunking, threading and output format as mg_points_decode / mg_points_encode.
 *      status, first match: uncompressed -- bit 7: BAD_ENCODING (`ExpectedUncompressed`); bit 6: OK (infinity) if the rest
 *      is zero, else BAD_ENCODING (`PointAtInfinity`); checked and off the curve: NOT_ON_CURVE; checked and [r]P != O:
 *      NOT_IN_SUBGROUP. compressed -- bit 6: as above (bit 7 beside it is ignored); x^3 + b without a root: NOT_ON_CURVE;
 *      checked and [r]P != O: NOT_IN_SUBGROUP. checked = 0 is legal for both forms (`deserialize_unchecked`; compressed:
 *      `deserialize_compressed`, which leaves the subgroup test to its caller). An all-zero record is not infinity: it is
 *      the point (0, 0) uncompressed and x = 0 compressed. ----------------------------------------------------------- */
int mg_ppot_points_decode(mg_curve_t curve, int group, const uint8_t *bytes, size_t n, int compressed, int checked,
                          uint64_t *out_affine_mont, uint8_t *status /* may be NULL */, size_t *n_bad /* may be NULL */);
/* n affine Montgomery points -> PPoT records back to back (`PpotSerializer::serialize_compressed` / `_uncompressed`):
 * infinity is byte 0 = 0x40 and zeros; compressed sets bit 7 when y > -y. */
int mg_ppot_points_encode(mg_curve_t curve, int group, const uint64_t *affine_mont, size_t n, int compressed, uint8_t *out);
/* Blake2b-512 (RFC 7693; unkeyed, no salt, no personalisation -- the reference's `Blake2b::default()`, the hash of a PPoT
 * file's 64-byte header and of a response): host code, any length. */
int mg_blake2b512(const uint8_t *data, size_t len, uint8_t out64[64]);

/* ---- batched Poseidon over the scalar field and the hashing of manta's UTXO Merkle forest. Replaces, in bulk,
 *      `Hasher<S, T, ARITY>::hash` (manta-pay/src/crypto/poseidon/hash.rs:111-153) and the Poseidon permutation
 *      (poseidon/mod.rs:383-419), and the inner hashing of `merkle_tree::Full` (root, `Path`) of manta-pay's UTXO accumulator
 *      (config/utxo.rs:1200-1301): one state per GPU lane. Field elements are Montgomery limbs (4 x u64) of Fr of `curve`.
 *      Synchronous, thread-safe and re-entrant, on the calling thread's setup stream. permute / hash run at most
 *      MG_POSEIDON_CHUNK states at a time: device memory of a call < MG_POSEIDON_CHUNK x 192 B (96 MiB) + the parameters,
 *      whatever n, and no pinned host memory. A tree and a forest keep every level on the device (about 2 x their leaves x
 *      32 B: 64 MB for 2^20 leaves). ------------------------------------------------------------------------------------- */
#define MG_POSEIDON_CHUNK (1u << 19)
typedef struct mg_poseidon mg_poseidon; /* a decoded parameter set (host memory only: creating one needs no GPU) */
/* bytes = the manta codec of `Hasher<S, T, ARITY>` (hash.rs:155-192, mod.rs:465-506): (full_rounds + partial_rounds) x width
 * additive round keys, the width x width MDS matrix row-major, the domain tag; 32-byte little-endian canonical elements each.
 * MG_ERROR_INVALID_ARGUMENT, with nothing allocated, for width outside 3..6, full_rounds odd or <= 0, partial_rounds < 0, a
 * length that does not match, or an element >= r. */
int mg_poseidon_create(mg_curve_t curve, int width, int full_rounds, int partial_rounds, const uint8_t *bytes, size_t len,
                       mg_poseidon **out);
void mg_poseidon_destroy(mg_poseidon *h);
/* n states of `width` words each, permuted in place */
int mg_poseidon_permute(const mg_poseidon *h, uint64_t *states_mont, size_t n);
/* n x (width - 1) inputs -> n digests: word 0 of the permutation of (domain tag, inputs) */
int mg_poseidon_hash(const mg_poseidon *h, const uint64_t *inputs_mont, size_t n, uint64_t *out_mont);
/* the same on HBM pointers (as mg_ntt_device), whole batch in one launch */
int mg_poseidon_hash_device(const mg_poseidon *h, const uint64_t *d_inputs_mont, size_t n, uint64_t *d_out_mont);
/* A tree of `height` (2..32) with n <= 2^(height - 1) leaves inserted left to right (leaf hash = identity, utxo.rs:1188);
 * h must have width 3. A node whose subtree holds no leaf is 0, every other node is hash(left, right) with an absent child
 * = 0. root_out: 4 limbs (0 for n = 0). For each of the k indices (< n) paths_out gets manta's `Path`: the leaf sibling,
 * then the height - 2 inner siblings bottom-up, height - 1 digests in all, absent siblings = 0. */
int mg_merkle_tree(const mg_poseidon *h, unsigned height, const uint64_t *leaves_mont, size_t n, uint64_t *root_out,
                   const uint64_t *indices, size_t k, uint64_t *paths_out);
/* n_trees trees of `height` at once: tree i holds leaves offsets[i] .. offsets[i + 1] - 1 (offsets[0] = 0, non-decreasing,
 * at most 2^(height - 1) each) -> roots_out[i]. Routing leaves to trees stays with the caller (utxo.rs:1319-1337). */
int mg_merkle_forest_roots(const mg_poseidon *h, unsigned height, const uint64_t *leaves_mont, const uint64_t *offsets,
                           size_t n_trees, uint64_t *roots_out);
/* Appending to trees that are known only by their current path, as `merkle_tree::single_path::SinglePath` (the ledger's
 * forest) and `Partial::from_leaves_and_path` (the signer's) keep them; replaces the hashing of `Tree::extend_digests` /
 * `batch_push` (tree.rs:351-406) and `CurrentInnerPath::update` (path.rs:416), 19 dependent hashes per leaf there.
 * The state of tree i: counts[i] = its leaves so far (n_old) and, for n_old > 0, leaf n_old - 1 and that leaf's `Path`
 * exactly as mg_merkle_tree(..., indices = [n_old - 1]) returns it (`CurrentPath` with its sentinels written out: an entry
 * on a level where bit l of n_old - 1 is 0 is a right sibling and must be 0). For n_old = 0 both are ignored. */
typedef struct mg_merkle_state { /* n_trees trees, a struct of arrays */
    uint64_t *counts;            /* [n_trees] */
    uint64_t *last_leaves;       /* [n_trees][4] */
    uint64_t *current_paths;     /* [n_trees][height - 1][4] */
} mg_merkle_state;
/* Tree i gets leaves offsets[i] .. offsets[i + 1] - 1 appended (offsets as for mg_merkle_forest_roots; b = 0 is allowed,
 * n_old + b <= 2^(height - 1)). roots_out[i] and new_state (the state of leaf n_new - 1; unchanged for b = 0; new_state may
 * be old_state, its arrays are the caller's) equal what mg_merkle_tree gives over all n_new leaves, bit for bit, and so do
 *   paths_out [k][height - 1][4]: the `Path` in the new tree of new leaf path_indices[q] (n_old <= index < n_new) of tree
 *     path_trees[q];
 *   refresh_paths_inout [m][height - 1][4]: on entry the `Path` of older leaf refresh_indices[q] (< n_old) of tree
 *     refresh_trees[q] in the old tree, on return its `Path` in the new one: only the entries whose sibling was recomputed
 *     are overwritten.
 * Only the nodes n_old >> l .. ceil(n_new / 2^l) - 1 of each level l are computed. Device memory of a call follows the
 * appended work, not the trees' sizes: about (2 B + n_trees x height) x 32 B for B appended leaves in all, plus the states
 * (n_trees x (height + 1) x 32 B) and the requests ((k + m) x height x 32 B).
 * h must have width 3, height 2..32. MG_ERROR_INVALID_ARGUMENT, before any device work and with nothing written: a null array
 * with a non-zero count, offsets not from 0 or decreasing, a tree over capacity, a request's tree >= n_trees or index outside
 * its range, a non-zero right sibling in a current path. n_trees = 0 succeeds. */
int mg_merkle_forest_append(const mg_poseidon *h, unsigned height, size_t n_trees, const mg_merkle_state *old_state,
                            const uint64_t *leaves_mont, const uint64_t *offsets, uint64_t *roots_out,
                            mg_merkle_state *new_state, const uint64_t *path_trees, const uint64_t *path_indices, size_t k,
                            uint64_t *paths_out, const uint64_t *refresh_trees, const uint64_t *refresh_indices, size_t m,
                            uint64_t *refresh_paths_inout);

/* ---- manta-pay's embedded curve and its Poseidon note encryption, one point / note per GPU lane. The curve is
 *      `ed_on_bn254` (`Group = ed_on_bn254::EdwardsProjective`, manta-pay/src/config/mod.rs): a x^2 + y^2 = 1 + d x^2 y^2 over
 *      BN254 Fr with a = 1, d = 168696 / 168700, cofactor 8, subgroup of prime order l (251 bits). Replaces, in bulk, ark-ec
 *      0.3 `twisted_edwards_extended::{GroupAffine, GroupProjective}` (add, mul, CanonicalSerialize / CanonicalDeserialize,
 *      `is_in_correct_subgroup_assuming_on_curve`) as used by address derivation and `StandardDiffieHellman` key agreement
 *      (manta-accounting/src/transfer/utxo/protocol.rs:1396-1451), and `IncomingBaseEncryptionScheme` =
 *      `FixedDuplexer<1, Poseidon3>` (manta-pay/src/config/utxo.rs:564-758, manta-pay/src/crypto/poseidon/encryption.rs,
 *      manta-crypto/src/permutation/duplex.rs). Only MG_BN254; MG_BLS12_381 is MG_ERROR_INVALID_ARGUMENT.
 *      Points are affine x | y Montgomery limbs of BN254 Fr (8 x u64), the identity is (0, 1). Embedded scalars are 4 x u64
 *      canonical little-endian integers below l; a scalar >= l is MG_ERROR_INVALID_ARGUMENT (checked on the host before any
 *      device work). The addition law is complete on the curve (d is a non-square), so points of small order need no special
 *      case; input points that are not on the curve give meaningless output (mg_edwards_check tells). Synchronous,
 *      thread-safe, on the calling thread's setup stream, MG_EDWARDS_CHUNK lanes at a time (device memory of a call < 32 MiB
 *      whatever n); n = 0 succeeds.
 *      Encoding (32 bytes): x little-endian canonical with bit 255 set iff y > -y as integers in [0, p) -- the ark-ec 0.3
 *      layout, which manta-parameters' group-generator.dat confirms. x = 0 decodes to the identity whatever the flag and the
 *      identity encodes as zeros, so the point of order two (0, -1) does not survive a round trip; this x = 0 rule restates
 *      ark-ec 0.3's serializer from memory and is not confirmed by any file of the reference. ------------------------------ */
#define MG_EDWARDS_CHUNK (1u << 16)
/* n encodings -> n points and status[i] = MG_POINT_*: x >= p (with bit 255 cleared) is MG_POINT_BAD_ENCODING; no square root
 * for y^2 = (1 - x^2) / (1 - d x^2) is MG_POINT_NOT_ON_CURVE; [l]P != O is MG_POINT_NOT_IN_SUBGROUP; checked = 0 skips only
 * the subgroup test. A rejected point is returned as zeros. status and n_bad (rejected count) may be NULL. */
int mg_edwards_decode(mg_curve_t curve, const uint8_t *bytes, size_t n, int checked, uint64_t *out_affine_mont, uint8_t *status,
                      size_t *n_bad);
/* n points -> n encodings of 32 bytes */
int mg_edwards_encode(mg_curve_t curve, const uint64_t *affine_mont, size_t n, uint8_t *out);
/* points in memory: a coordinate >= p, then the curve equation, then the subgroup, with the same statuses */
int mg_edwards_check(mg_curve_t curve, const uint64_t *affine_mont, size_t n, uint8_t *status, size_t *n_bad);
#define MG_EDWARDS_MUL_SHARED_SCALAR 0 /* n_scalars = 1: out[i] = points[i] * scalar (key agreement), n_points results */
#define MG_EDWARDS_MUL_FIXED_BASE 1    /* n_points = 1: out[i] = point * scalars[i] (key derivation), n_scalars results */
#define MG_EDWARDS_MUL_PAIRWISE 2      /* n_points = n_scalars: out[i] = points[i] * scalars[i] */
int mg_edwards_mul(mg_curve_t curve, int mode, const uint64_t *points_affine_mont, size_t n_points, const uint64_t *scalars,
                   size_t n_scalars, uint64_t *out_affine_mont);
/* out[i] = a[i] + b[i] */
int mg_edwards_add(mg_curve_t curve, const uint64_t *a_affine_mont, const uint64_t *b_affine_mont, size_t n,
                   uint64_t *out_affine_mont);

/* The incoming-note cipher. bytes = manta-parameters' incoming-base-encryption-scheme.dat (8 712 bytes): the width-4
 * permutation (8 full and 55 partial rounds: 63 x 4 round keys, the 4 x 4 MDS matrix, no domain tag), a u64 4 and the four
 * elements of `FixedEncryption::initial_state`, 32-byte little-endian canonical elements. generator = the group generator G
 * (group-generator.dat decoded). Host only, no GPU needed: MG_ERROR_INVALID_ARGUMENT, with nothing allocated, for any other
 * length, an element >= p, or a generator that is not on the curve. */
typedef struct mg_note_cipher mg_note_cipher;
int mg_note_cipher_create(mg_curve_t curve, const uint8_t *bytes, size_t len, const uint64_t *generator_affine_mont,
                          mg_note_cipher **out);
void mg_note_cipher_destroy(mg_note_cipher *h);
/* `Hybrid` encryption of n notes: epk[i] = G * randomness[i], the sponge is keyed by (x, y) of recv_keys[i] * randomness[i];
 * plaintexts / ciphertexts are 3 Montgomery elements per note (commitment randomness, asset id, asset value), tags one. The
 * sponge: state <- initial state; words 1..3 += (x, y, 0), permute; permute again (the empty header is one all-zero setup
 * block: manta-util/src/vec.rs `padded_chunks_with`); words 1..3 += plaintext = the ciphertext, permute; tag = word 1. */
int mg_notes_encrypt(const mg_note_cipher *h, const uint64_t *recv_keys_affine_mont, const uint64_t *randomness,
                     const uint64_t *plaintexts_mont, size_t n, uint64_t *epk_out_affine_mont, uint64_t *ciphertext_out_mont,
                     uint64_t *tag_out_mont);
#define MG_NOTE_OK 0
#define MG_NOTE_BAD_TAG 1   /* the recomputed tag differs: not this key's note, or altered */
#define MG_NOTE_BAD_VALUE 2 /* the tag matches but the asset value word is 2^128 or more (`try_into_u128`, utxo.rs:716-731) */
/* Decryption of n Poseidon notes against one viewing key: the sponge is keyed by epks[i] * viewing_key; ok[i] = 1 iff the note
 * opens (status[i] = MG_NOTE_OK; status may be NULL), and the plaintext of a note that does not is zeros. (The scan a wallet
 * runs, `NoteOpen::open`, reads the light note and not this one: mg_light_notes_open below.) */
int mg_notes_decrypt(const mg_note_cipher *h, const uint64_t *viewing_key, const uint64_t *epks_affine_mont,
                     const uint64_t *ciphertexts_mont, const uint64_t *tags_mont, size_t n, uint64_t *plaintext_out_mont,
                     uint8_t *ok, uint8_t *status);

/* ---- manta-pay's UTXO statement, one UTXO or one key per GPU lane: commitments, accumulator items, nullifier commitments and
 *      viewing keys. Replaces, in bulk, `utxo_reconstruct` / `utxo_check` (manta-accounting/src/transfer/utxo/protocol.rs:
 *      1461-1499), `item_hash` (manta-pay/src/config/utxo.rs:1153-1167), the commitment, record and item of `derive_mint`
 *      (protocol.rs:1152-1207), the nullifier commitment of `derive_spend` (protocol.rs:1291-1350) and
 *      `ViewingKeyDerivationFunction::viewing_key` (utxo.rs:523-545). Only MG_BN254; MG_BLS12_381 is MG_ERROR_INVALID_ARGUMENT.
 *      With H5, H4, H3, H2 the `Hasher`s of utxo-commitment-scheme.dat (width 6, 8 + 56 rounds), utxo-accumulator-item-hash.dat
 *      (width 5, 8 + 56), nullifier-commitment-scheme.dat (width 4, 8 + 55) and viewing-key-derivation-function.dat (width 3,
 *      8 + 55), hash = word 0 of the permutation of (tag, inputs):
 *        UTXO record  = flag | public id | public value | commitment, four Montgomery elements; flag 0 opaque, 1 transparent
 *        plaintext    = randomness | asset id | asset value, the three elements of the notes calls
 *        secret asset = the asset when opaque, (0, 0) when transparent; public asset = the reverse (protocol.rs:93-114)
 *        commitment   = H5 of randomness, secret id, secret value, rk.x, rk.y              (utxo.rs:367-393)
 *        item         = H4 of flag, public id, public value, commitment                    (utxo.rs:1153-1167)
 *        nullifier    = H3 of pak.x, pak.y, item                                           (utxo.rs:1465-1485)
 *        viewing key  = H2 of pak.x, pak.y as an integer mod l (`rem_mod_prime`); receiving key = viewing key * G
 *      Elements are Montgomery limbs of BN254 Fr, points affine x | y (8 x u64), embedded scalars 4 x u64 canonical below l, as
 *      in the calls above. Per-lane status: MG_UTXO_BAD_ENCODING for a flag that is not 0 / 1 or an asset value or public value
 *      word of 2^128 or more (`AssetValue` is a u128 and `is_transparent` a bool by type), else MG_UTXO_MISMATCH (open only);
 *      a lane that is not MG_UTXO_OK returns zeros in every output of that lane. The nullifier commitments of items already at
 *      hand need no call of their own: that is the hash call of a width-4 mg_poseidon handle over rows pak.x | pak.y | item.
 *      Synchronous, thread-safe (a model is immutable host memory; the constants are uploaded per call), on the calling thread's
 *      setup stream, MG_EDWARDS_CHUNK lanes at a time (device memory of a call < 32 MiB whatever n); n = 0 succeeds. ---------- */
#define MG_UTXO_OK 0
#define MG_UTXO_BAD_ENCODING 1
#define MG_UTXO_MISMATCH 2 /* the rebuilt record differs from the ledger's in a public word or in the commitment */
typedef struct mg_utxo_file {
    const uint8_t *bytes;
    size_t len;
} mg_utxo_file;
typedef struct mg_utxo_files { /* manta-parameters' files of the fields of `BaseParameters` (protocol.rs:530-570), each whole */
    mg_utxo_file utxo_commitment_scheme;
    mg_utxo_file utxo_accumulator_item_hash;
    mg_utxo_file nullifier_commitment_scheme;
    mg_utxo_file viewing_key_derivation_function;
    mg_utxo_file group_generator; /* 32 bytes, the encoding mg_edwards_decode reads */
} mg_utxo_files;
typedef struct mg_utxo_model mg_utxo_model;
/* Decodes these five files with the manta codec. Host only, no GPU needed: MG_ERROR_INVALID_ARGUMENT, with nothing allocated, for
 * a length that is not exactly the file's, an element >= r, or a generator that does not decode, is the identity, is off the
 * curve or outside the subgroup of order l. The fixed-base table of G is built here, once per model. */
int mg_utxo_model_create(mg_curve_t curve, const mg_utxo_files *files, mg_utxo_model **out);
void mg_utxo_model_destroy(mg_utxo_model *h);
/* The sender's side of `derive_mint`: plaintexts hold the whole asset, flags[i] (a byte, 0 / 1) says which half is secret ->
 * the records (n x 16 u64), their items (n x 4) and status[i] = MG_UTXO_OK / MG_UTXO_BAD_ENCODING. With mg_notes_encrypt,
 * mg_light_notes_encrypt and mg_address_partitions this is the whole of `derive_mint`. Every array must be given. */
int mg_utxos_mint(const mg_utxo_model *h, const uint64_t *recv_keys_affine_mont, const uint64_t *plaintexts_mont,
                  const uint8_t *flags, size_t n, uint64_t *utxos_out_mont, uint64_t *items_out_mont, uint8_t *status);
/* The receiver's side: `utxo_check` of n opened notes against the ledger's records for the address viewing_key * G (computed
 * once per call), the identifier being (the record's flag, the plaintext's randomness); then `item_hash`, and -- when pak (one
 * affine point on the curve) and nullifiers_out are both given; one without the other is an invalid argument -- the nullifier
 * commitment. *n_ok (may be NULL) = the number of MG_UTXO_OK lanes. A viewing key >= l or a pak off the curve is
 * MG_ERROR_INVALID_ARGUMENT before any device work. */
int mg_utxos_open(const mg_utxo_model *h, const uint64_t *viewing_key, const uint64_t *pak_affine_mont,
                  const uint64_t *plaintexts_mont, const uint64_t *utxos_mont, size_t n, uint8_t *status, uint64_t *items_out_mont,
                  uint64_t *nullifiers_out_mont, size_t *n_ok);
/* n proof authorization keys -> their viewing keys (canonical limbs below l) and, unless NULL, the receiving keys (affine
 * Montgomery): the account table of a signer. The keys' coordinates must be reduced; they are hashed as given. */
int mg_viewing_keys(const mg_utxo_model *h, const uint64_t *paks_affine_mont, size_t n, uint64_t *viewing_keys_out,
                    uint64_t *recv_keys_out_affine_mont);

/* ---- Batched Schnorr authorization signatures of manta-pay: the `AuthorizationSignature` of every `TransferPost` that spends
 *      (manta-crypto/src/signature/mod.rs `schnorr::{sign, verify}`, manta-pay/src/config/utxo.rs `SchnorrHashFunction`,
 *      manta-accounting/src/transfer/utxo/protocol.rs `signature_scheme()` and `auth::VerifySignature::verify`). The generator
 *      is `base.group_generator`, the G of the model above: the calls take its handle and need no parameter file of their own
 *      (schnorr-hash-function.dat is empty). One signature per lane:
 *        challenge  h = Blake2s-256("manta-pay/1.0.0/Schnorr-hash" | enc(pk) | enc(R) | message) as a little-endian integer,
 *                   reduced mod l (`from_le_bytes_mod_order`); enc = the 32 bytes mg_edwards_encode writes
 *        sign       R = k G, pk = sk G, s = k + sk h mod l; the signature is (s, R). Deterministic given the nonce k.
 *        verify     the ledger's rule: s G == R is refused (MG_SIG_DEGENERATE; it happens exactly when sk h = 0 mod l, e.g.
 *                   sk = 0), otherwise accepted iff s G == R + h pk
 *      Points are affine x | y Montgomery (8 x u64), scalars and challenges 4 x u64 canonical below l, as in the calls above.
 *      Messages cross as n rows of `stride` bytes, row i at messages + i * stride, with lengths[i] <= stride bytes of it the
 *      message (the rest is never hashed); lengths = NULL: every message is `stride` bytes. stride is a multiple of 4, at
 *      most MG_SIGNATURE_MAX_MESSAGE; stride = 0 is legal (empty messages; `messages` may then be NULL).
 *      Per-lane status of a verification, in this order of precedence: MG_SIG_BAD_ENCODING for s >= l (it comes off the wire), a
 *      coordinate >= p, or pk or R not on the curve -- the subgroup test stays with mg_edwards_decode, whose rejected lanes
 *      arrive here as (0, 0) and are refused --, MG_SIG_DEGENERATE, MG_SIG_MISMATCH, MG_SIG_OK.
 *      MG_ERROR_INVALID_ARGUMENT before any device work: a NULL required array, a stride that is not a multiple of 4 or above
 *      the maximum, a lengths[i] > stride, and for signing a key or nonce >= l (the caller's own secrets). n = 0 succeeds.
 *      Synchronous, thread-safe, on the calling thread's setup stream, nothing on the NULL stream; the model's table (94.5 KB)
 *      is uploaded once per call. Lanes per device pass = min(2^16, max(64, 16 MiB / max(stride, 4))): a pass holds at most
 *      16 MiB of message rows and 16.25 MiB of everything else, so the device memory of a call is < 33 MiB whatever n and
 *      stride. ------------------------------------------------------------------------------------------------------------- */
#define MG_SIGNATURE_MAX_MESSAGE (1u << 16)
#define MG_SIG_OK 0
#define MG_SIG_BAD_ENCODING 1
#define MG_SIG_DEGENERATE 2 /* s G == R: refused by `VerifySignature::verify` before the equation is looked at */
#define MG_SIG_MISMATCH 3
/* The challenges alone (n x 4 u64). The points are encoded as given: reduced coordinates are the caller's business here. */
int mg_schnorr_challenges(const mg_utxo_model *h, const uint64_t *pks_affine_mont, const uint64_t *nonce_points_affine_mont,
                          const uint8_t *messages, size_t stride, const uint32_t *lengths, size_t n, uint64_t *challenges_out);
/* n signatures (scalars[i], nonce_points[i]) of messages[i] under pks[i] -> status[i] (may be NULL) and *n_ok (may be NULL) =
 * the number of MG_SIG_OK lanes. Beside mg_groth16_verify_batch a ledger chains mg_edwards_decode -> mg_signatures_verify. */
int mg_signatures_verify(const mg_utxo_model *h, const uint64_t *pks_affine_mont, const uint64_t *nonce_points_affine_mont,
                         const uint64_t *scalars, const uint8_t *messages, size_t stride, const uint32_t *lengths, size_t n,
                         uint8_t *status, size_t *n_ok);
/* n signatures with the caller's keys and nonces (both < l) -> scalars (n x 4), nonce points (n x 8) and, unless NULL, the
 * verifying keys sk G (n x 8). */
int mg_signatures_sign(const mg_utxo_model *h, const uint64_t *signing_keys, const uint64_t *nonces, const uint8_t *messages,
                       size_t stride, const uint32_t *lengths, size_t n, uint64_t *scalars_out,
                       uint64_t *nonce_points_out_affine_mont, uint64_t *pks_out_affine_mont);

/* ---- manta-pay's AES-GCM notes, its address partition and its Merkle shard index, one note, key or leaf per GPU lane. What
 *      `NoteOpen::open` (manta-accounting/src/transfer/utxo/protocol.rs:1396-1434), `NullifierOpen::open` (1371-1394) and the
 *      note halves of `derive_mint` / `derive_spend` (1330-1340) run: `IncomingBaseAES` and `OutgoingBaseAES`
 *      (manta-pay/src/config/utxo.rs:760-1031, 1511-1777; manta-pay/src/crypto/encryption/aes.rs), `AddressPartitionFunction`
 *      (utxo.rs:1810-1831) and the shard function of the UTXO Merkle forest (utxo.rs:1319-1337). Only MG_BN254. The handle is
 *      the UTXO model above: the calls use its generator table and need no parameter file of their own.
 *        key        = Blake2s-256(enc(K)), K the agreed point: recv_key * randomness when encrypting, epk * viewing_key when
 *                     opening; enc = the 32 bytes mg_edwards_encode writes. Keys and agreed points never leave the device.
 *        cipher     = AES-256-GCM, nonce "random nonce" (12 bytes), no associated data; a note crosses as ciphertext | tag
 *        light note = randomness | asset id (32 bytes little-endian canonical each) | asset value (u128, 16 bytes little-endian):
 *                     80 -> MG_LIGHT_NOTE_BYTES; across this ABI the plaintext is the three Montgomery elements of the Poseidon
 *                     note calls, and the ephemeral key is that note's (`light_incoming_randomness()` clones the randomness)
 *        outgoing   = asset id | asset value: 48 -> MG_OUTGOING_NOTE_BYTES; two Montgomery elements per note; it is sealed to
 *                     the spender's own receiving key, one per call
 *        partition  = Blake2s with a ONE-byte digest over "manta-v1.0.0/address-partition-function" | x | y of the receiving
 *                     key, 32 bytes little-endian canonical each (`serialize_unchecked` of the affine point). That this is plain
 *                     x | y with no flag bits, the identity (0, 1) included, restates ark-ec 0.3 from memory and is not
 *                     confirmed by any file of the reference.
 *        shard      = the same hash over "manta-v1.0.0/merkle-tree-shard-function" | leaf: the byte a caller needs per leaf
 *                     to build the `offsets` of mg_merkle_forest_roots
 *      Per-lane status: the MG_NOTE_* above and MG_NOTE_OTHER_PARTITION. MG_NOTE_BAD_VALUE when encrypting is a value word of
 *      2^128 or more; when opening it is a verified tag over randomness or id bytes that are not below r (the reference
 *      `.expect()`s there). A lane that is not MG_NOTE_OK returns zeros in every output of that lane.
 *      MG_ERROR_INVALID_ARGUMENT before any device work: a NULL required array or model, a randomness or viewing key >= l, the
 *      outgoing receiving key off the curve or unreduced, an n whose arrays would wrap a size_t. Coordinates of the other
 *      points must be reduced; points off the curve give meaningless notes (mg_edwards_check tells). n = 0 succeeds.
 *      Synchronous, thread-safe, on the calling thread's setup stream, nothing on the NULL stream, MG_EDWARDS_CHUNK lanes at a
 *      time (device memory of a call < 32 MiB whatever n). ------------------------------------------------------------------ */
#define MG_NOTE_OTHER_PARTITION 3 /* mg_light_notes_open with partitions: the note carries another address's byte; not tried */
#define MG_LIGHT_NOTE_BYTES 96
#define MG_OUTGOING_NOTE_BYTES 64
/* n receiving keys (n x 8 u64) -> n bytes; n leaves (n x 4 u64 Montgomery) -> n bytes */
int mg_address_partitions(const mg_utxo_model *h, const uint64_t *recv_keys_affine_mont, size_t n, uint8_t *out);
int mg_merkle_shard_indices(mg_curve_t curve, const uint64_t *leaves_mont, size_t n, uint8_t *out);
/* The light note of `derive_mint`: n notes (n x MG_LIGHT_NOTE_BYTES) and status[i] = MG_NOTE_OK / MG_NOTE_BAD_VALUE; the
 * ephemeral keys G * randomness[i], unless NULL, equal those of mg_notes_encrypt for the same randomness. Every other array
 * must be given. */
int mg_light_notes_encrypt(const mg_utxo_model *h, const uint64_t *recv_keys_affine_mont, const uint64_t *randomness,
                           const uint64_t *plaintexts_mont, size_t n, uint64_t *epk_out_affine_mont /* may be NULL */,
                           uint8_t *ciphertexts_out, uint8_t *status);
/* `NoteOpen::open` of n ledger notes against one viewing key. With `partitions` (the notes' partition bytes) the call computes
 * its own byte once on the host (viewing_key * G from the model's table, then the hash), and only the lanes that carry it go
 * through a key agreement and the cipher: they are gathered before the device passes. Every other lane is
 * MG_NOTE_OTHER_PARTITION whatever its ciphertext holds. partitions = NULL tries every lane. ok[i] = 1 iff status[i] =
 * MG_NOTE_OK (status may be NULL); *n_tried (may be NULL) = the lanes that went through a key agreement. */
int mg_light_notes_open(const mg_utxo_model *h, const uint64_t *viewing_key, const uint64_t *epks_affine_mont,
                        const uint8_t *ciphertexts, const uint8_t *partitions /* may be NULL */, size_t n,
                        uint64_t *plaintext_out_mont, uint8_t *ok, uint8_t *status, size_t *n_tried /* may be NULL */);
/* The outgoing note of `derive_spend`, sealed to ONE receiving key (the spender's own): its fixed-base table is built on the
 * host for the call, so both products of a lane are table products. Every array must be given. */
int mg_outgoing_notes_encrypt(const mg_utxo_model *h, const uint64_t *recv_key_affine_mont /* one */, const uint64_t *randomness,
                              const uint64_t *assets_mont, size_t n, uint64_t *epk_out_affine_mont, uint8_t *ciphertexts_out,
                              uint8_t *status);
/* `NullifierOpen::open`: n outgoing notes against one viewing key -> the assets (n x 8 u64); status may be NULL */
int mg_outgoing_notes_open(const mg_utxo_model *h, const uint64_t *viewing_key, const uint64_t *epks_affine_mont,
                           const uint8_t *ciphertexts, size_t n, uint64_t *assets_out_mont, uint8_t *ok, uint8_t *status);

#ifdef __cplusplus
}
#endif
#endif
