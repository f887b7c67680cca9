/* mi355_msm.h -- C ABI of the MI355X (gfx950) multi-scalar-multiplication engine.
 *
 * This is the drop-in boundary for the ZPrize-2022 prize1-msm hot path: plain pointers and sizes,
 * no C++ or torch types.  Every entry point names the reference interface it replaces
 * (paths relative to /root/reference, abbreviations as in SURVEY.md):
 *
 *   SPK  = open-division/prize1-msm/prize1a-msm-gpu/6block/sppark
 *   P1A  = open-division/prize1-msm/prize1a-msm-gpu
 *   CMB  = P1A/combined-top-solutions/combined-msm
 *   ARK  = open-division/prize4-msm-wasm/snarkify/zprize-prize4-15ac8c55-arkworks-algebra
 *
 * Data layouts (identical to what the reference FFI passes):
 *   bases    arkworks `Affine` images: x, y as 6 x u64 little-endian Montgomery (R = 2^384) limbs,
 *            then a 1-byte infinity flag; element stride is passed explicitly (104 B for G1).
 *            The flag byte is authoritative for infinity, not the coordinates.
 *   scalars  32 B each, 4 x u64 little-endian, plain integers (`BigInteger256`).
 *   results  arkworks `Projective` images (Jacobian X, Y, Z; 3 x 48 B Montgomery; 3 x 96 B for G2), written NORMALISED:
 *            (x, y, 1), or (1, 1, 0) for the point at infinity -- so equal points are equal bytes.
 *
 * Errors: `RustError { int code; char *message; }` returned by value, exactly sppark's convention
 * (SPK util/rusterror.h:15-27): code 0 = success, otherwise a hipError_t value (or -1 for argument
 * errors) and a malloc'd message the caller frees (Rust side: SPK rust/src/lib.rs:17-25).  A message is
 * ALWAYS supplied on failure, because ROCm has no cudaGetErrorString for the Rust macro to fall back on.
 * No C++ exception crosses this boundary.
 *
 * There is no CPU fallback: every compute entry point needs a visible gfx950 device and fails with
 * hipErrorNoDevice otherwise.
 */
#ifndef MI355_MSM_H
#define MI355_MSM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
  int code;
  char* message;
} RustError;

typedef struct mi355_msm_ctx mi355_msm_ctx;

enum {
  MI355_BLS12_377_G1 = 0, /* fq: ARKC bls12_377/src/fields/fq.rs:4, curve b = 1 */
  MI355_BLS12_381_G1 = 1, /* fq: ARKC bls12_381/src/fields/fq.rs:4, curve b = 4 */
  MI355_BLS12_377_G2 = 2, /* coordinates in Fq2 = Fq[u]/(u^2+5) (ARKC bls12_377/src/fields/fq2.rs:13, curves/g2.rs:47-78):
                             Affine images are 200 B (x.c0 x.c1 y.c0 y.c1, flag at byte 192), Projective images 288 B */
  MI355_BLS12_381_G2 = 3  /* Fq2 = Fq[u]/(u^2+1), b' = 4(1+u) (ARKC bls12_381/src/fields/fq2.rs:13, curves/g2.rs:47-48, 74-91);
                             same images as MI355_BLS12_377_G2 */
};

/* Stage indices of mi355_msm_last_timings(). */
enum {
  MI355_T_DIGITS = 0,
  MI355_T_SORT = 1,
  MI355_T_ACCUMULATE = 2, /* the dominant kernel (bucket accumulation) */
  MI355_T_SEGREDUCE = 3,
  MI355_T_BUCKET_REDUCE = 4,
  MI355_T_HOST_FOLD = 5,
  MI355_T_TOTAL = 6,
  MI355_T_COUNT = 8
};

/* ---- canonical context API ---------------------------------------------------------------------
 * Replaces the context half of the harness FFI: mult_pippenger_init / mult_pippenger_inf
 * (P1A 6block/cuda/pippenger_inf.cu:50-53, 87-92) and MSMAllocContext / MSMPreprocessPoints / MSMRun /
 * MSMFreeContext (CMB MSM.h:72-75).  Bases are uploaded and converted once; each run streams scalars. */

/* device < 0 selects the current HIP device. */
RustError mi355_msm_create(mi355_msm_ctx** out, int curve, int device);
RustError mi355_msm_destroy(mi355_msm_ctx* ctx);

/* ---- one MSM over several GPUs, behind the SAME context API ----------------------------------------
 * The reference is single-device (SPK msm/pippenger.cuh:400-416 hard-codes device 0), but its harness only ever calls
 * init + run (P1A 6block/src/lib.rs:54-109; CMB MSM.h:72-75), so sharding has to live behind those calls.  A sharded context
 * is an ordinary mi355_msm_ctx*: set_bases / set_bases_device / set_bases_serialized / run / run_device / set_option / query /
 * last_timings / destroy all accept it.  Shard g of G owns the contiguous slice [g*ceil(n/G), ...) of the bases and of every
 * scalar batch, one host thread + one device context + one stream per shard (the multi-stream orchestration of
 * P1A matter-labs/src/lib.rs:125-201 with devices in place of streams); each shard's host thread returns one folded partial
 * point per batch, so the G partials are already in host memory and the "final 8-point curve add" is a host fold
 * (mi355_msm_fold) -- no collective is run by default.  Option "combine" = 2 additionally sends the partials through one
 * ncclAllGather over RCCL/xGMI (single-process communicator, built at set_bases; librccl is dlopen'ed) and requires the
 * exchanged copy to equal what was sent: a link check for bring-up, not a step the result depends on (0 / 1: host fold only).
 * The collective that IS needed -- partials in different processes -- is the one-process-per-GPU path (dist.py, torchrun).
 * Queries: "shards", "rccl_exchanges"; counters of the single-device queries add up over the shards. */
RustError mi355_msm_create_sharded(mi355_msm_ctx** out, int curve, const int* devices, int ndevices);
/* What the harness shims call: MI355_MSM_DEVICES = "0,1,2,3" | "0-7" | "all" selects a sharded context over those devices,
 * one entry (or unset) an ordinary one.  mi355_msm() (stateless) goes through here as well.
 * MI355_MSM_ASSUME_SUBGROUP = 0 | 1 sets the option "assume_subgroup" on the new context (the yrrid shim turns it on unless this says 0:
 * the reference it stands in for folds scalars with the top bit set, CMB ProcessSignedDigits.cu:123-128). */
RustError mi355_msm_create_env(mi355_msm_ctx** out, int curve);

/* Bases in HOST memory (arkworks Affine images, `stride` bytes apart).  Copies; caller keeps ownership. */
RustError mi355_msm_set_bases(mi355_msm_ctx* ctx, const void* affine, size_t npoints, size_t stride);
/* Same, bases already resident in DEVICE memory (e.g. a torch uint8 tensor's data_ptr). */
RustError mi355_msm_set_bases_device(mi355_msm_ctx* ctx, const void* d_affine, size_t npoints, size_t stride);

/* Are these points legal bases?  One status byte per point, decided on the context's device and stream; the context's own bases are
 * neither read nor changed.
 *   0  valid: flagged infinity, or on the curve and in the order-r subgroup
 *   1  a coordinate is not below p (in-memory image: the Montgomery limbs; serialized record: the integer after the two flag bits
 *      are masked)
 *   2  canonical, but y^2 != x^3 + b
 *   3  on the curve, outside the order-r subgroup
 * The infinity flag is authoritative (of a serialized record's flag bits only bit 6 is read: a record with both bits set, which arkworks
 * refuses, counts as infinity); the lowest applicable status wins.  This is what arkworks' checked reader does and
 * `deserialize_unchecked` skips (ARK ec/src/models/short_weierstrass.rs:67-77, 1204-1224); status 3 is decided by the endomorphism
 * tests of eprint 2021/1130 (ARKC bls12_381/src/curves/g1.rs:47-85, g2.rs:58-71) or, with flag bit 1, by [r]P == O itself --
 * identical verdicts (csrc/check_points.hpp argues why, for BLS12-377 as well).
 * flags: bit 0 = records are uncompressed CanonicalSerialize records (stride ignored), bit 1 = exact method.
 * status: HOST memory, npoints bytes, may be NULL.
 * out[8]: valid, of those flagged infinity, status 1, status 2, status 3, index of the first invalid point (npoints if none),
 *         method used (0 exact, 1 endomorphism), device microseconds (the check kernels alone, between events on the context's stream:
 *         neither the staging copies of host input nor the status copies back, so less than what the caller waits for).
 * Returns 0 when the check RAN, whatever it found; -1 for a sharded context, a stride too small or not a multiple of 4.
 * Option "validate_bases" = 1 (default 0; MI355_MSM_VALIDATE_BASES for mi355_msm_create_env) makes the three set_bases calls run
 * this check first: an invalid point fails the call with -1 and a message naming the first bad index and its status, and the
 * context keeps its previous bases.  Query "bases_validated": 1 when the current base set passed the check.
 * A sharded context refuses "validate_bases" = 1 (-1, from mi355_msm_set_option and so from mi355_msm_create_env when
 * MI355_MSM_VALIDATE_BASES=1 meets a list of several MI355_MSM_DEVICES): check on a single-device context first. */
RustError mi355_msm_check_bases(mi355_msm_ctx* ctx, const void* affine, size_t npoints, size_t stride, unsigned flags, uint8_t* status,
                                uint64_t* out);
RustError mi355_msm_check_bases_device(mi355_msm_ctx* ctx, const void* d_affine, size_t npoints, size_t stride, unsigned flags,
                                       uint8_t* status, uint64_t* out);

/* Bases as arkworks CanonicalSerialize UNCOMPRESSED records in host memory (row f2: what the harness persists with
 * `points.serialize_unchecked(File::create("points.bin"))`, P1B hardcaml/.../test_fpga_harness/src/util.rs:126-140): per point
 * x | y as little-endian normal-form integers (2 x 48 B for G1, 2 x 96 B for G2), SWFlags in the top two bits of the last
 * byte (bit 6 = infinity).  Pass the records WITHOUT the leading u64 element count.  Converted on the device. */
RustError mi355_msm_set_bases_serialized(mi355_msm_ctx* ctx, const void* records, size_t npoints);
/* The inverse for results: a Projective image (any Z) -> one uncompressed CanonicalSerialize record (host arithmetic),
 * comparable byte-for-byte with the harness's `arkworks_results.bin` entries. */
RustError mi355_msm_point_to_serialized(int curve, const void* projective, void* out_record);

/* arkworks COMPRESSED records -- what plain `serialize` / `deserialize` mean (ARK ec/src/models/short_weierstrass.rs:1120-1126,
 * 1188-1201), the form SRS files and proving keys ship in: x as a little-endian normal-form integer (48 B for G1; c0 | c1, 96 B,
 * for G2) with SWFlags in the top two bits of the last byte -- bit 6 infinity, bit 7 "y is the larger of y and -y" (Fp: the integer
 * exceeds (p - 1)/2; Fp2: c1 decides unless it is zero, then c0).  Decoded and encoded on the context's device and stream, in chunks
 * of option "codec_chunk" records (default 2^22) through buffers the context keeps; the context's bases are not touched.
 *
 * decompress: `records` -> `out`, npoints * stride bytes of arkworks in-memory Affine images (Montgomery R = 2^384, flag byte, every
 * pad byte of the stride written as zero, infinity as (0, 0, flag 1)), or with flags bit 0 npoints uncompressed records (stride
 * ignored; infinity as (0, 1) with bit 6, the record mi355_msm_point_to_serialized writes).  One status byte per record:
 *   0  decoded, or flagged infinity (the flag is authoritative: a flagged record is valid whatever its x bits hold)
 *   1  malformed: x (a component) is not below p after the flag bits are masked, or BOTH flag bits are set (arkworks refuses that
 *      encoding, and so does this decoder -- unlike the check of uncompressed records above, which stays lenient)
 *   2  no point has this x (x^3 + b has no square root)
 *   3  decoded, but outside the order-r subgroup -- only with flags bit 1, which runs mi355_msm_check_bases' kernel over the decoded
 *      records (flags bit 2: its exact method); a record that failed to decode keeps status 1 / 2
 * The lowest applicable status wins.  A record that fails is written as an all-zero record with flag 0, which mi355_msm_check_bases
 * reports as off the curve: never a silent infinity.
 * status: HOST memory, npoints bytes, may be NULL.  out8: laid out like mi355_msm_check_bases' out -- valid, of those flagged infinity,
 * status 1, 2, 3, index of the first failing record (npoints if none), method of the subgroup check (0 exact or none, 1 endomorphism),
 * device microseconds of the codec kernels alone (no copies, no subgroup check).
 * _device: `d_records` and `d_out` are device memory of the context's device, 4-byte aligned; nothing but the status bytes is staged.
 *
 * compress: images `stride` bytes apart, or with flags bit 0 uncompressed records, -> npoints compressed records.  Status 1 for a
 * non-canonical coordinate (the record is then all zeros); no curve test -- arkworks' `serialize` has none.
 *
 * Both return 0 when the codec RAN, whatever it found; -1 for a sharded context, unknown flags, a stride too small or not a multiple of 4. */
RustError mi355_msm_decompress_points(mi355_msm_ctx* ctx, const void* records, size_t npoints, void* out, size_t stride, unsigned flags,
                                      uint8_t* status, uint64_t* out8);
RustError mi355_msm_decompress_points_device(mi355_msm_ctx* ctx, const void* d_records, size_t npoints, void* d_out, size_t stride,
                                             unsigned flags, uint8_t* status, uint64_t* out8);
RustError mi355_msm_compress_points(mi355_msm_ctx* ctx, const void* points, size_t npoints, size_t stride, unsigned flags, void* out_records,
                                    uint8_t* status, uint64_t* out8);
RustError mi355_msm_compress_points_device(mi355_msm_ctx* ctx, const void* d_points, size_t npoints, size_t stride, unsigned flags,
                                           void* d_out_records, uint8_t* status, uint64_t* out8);
/* Bases as compressed records in host memory (WITHOUT a leading element count): decoded on the device, then handed to the path of
 * mi355_msm_set_bases_device, so tables, the Edwards conversion, the anchored sum and option "validate_bases" behave as for any other
 * input.  A record with a non-zero decode status fails the call with -1 and a message naming the first bad index and its status;
 * the context keeps its previous bases.  A sharded context refuses the call (-1). */
RustError mi355_msm_set_bases_compressed(mi355_msm_ctx* ctx, const void* records, size_t npoints);
/* A Projective image (any Z) -> one compressed record (host arithmetic), beside mi355_msm_point_to_serialized. */
RustError mi355_msm_point_to_compressed(int curve, const void* projective, void* out_record);

/* `batches` MSMs over the SAME bases: scalars holds batches * npoints entries, out receives `batches`
 * projective images (P1A 6block/src/lib.rs:85-109: batch_size = scalars.len() / points.len()).
 * npoints may be smaller than the number of uploaded bases (prefix). */
RustError mi355_msm_run(mi355_msm_ctx* ctx, void* out_projective, const void* scalars, size_t npoints, size_t batches);
/* Scalars already in DEVICE memory; `stream` is the hipStream_t on which the scalars become ready and on which all work is
 * enqueued (NULL = the HIP default stream, i.e. ordered after whatever a framework's default stream produced).  `out_projective` is HOST memory; the call returns
 * after the result is written (one stream synchronisation per batch chunk). */
RustError mi355_msm_run_device(mi355_msm_ctx* ctx, void* out_projective, const void* d_scalars, size_t npoints,
                               size_t batches, void* stream);

/* ---- stream-ordered run -------------------------------------------------------------------------------------------------
 * Replaces the asynchronous half of the second-place entry's API: msm_configuration.stream, h2d_copy_finished{,_callback},
 * d2h_copy_finished{,_callback} and msm_execute_async (ML bellman-cuda.h:48-75, ML msm.cu:97-468; caller:
 * P1A matter-labs/src/lib.rs:150-190), which lets a prover keep its own kernels (NTTs) running while an MSM is in flight.
 *
 * mi355_msm_run_async returns as soon as the job is queued (no device synchronisation in the calling thread).  The MSM is ordered
 * AFTER everything enqueued in `stream` before the call (an event is recorded there; `d_scalars` must be valid from that point
 * until the job has finished) and runs on the context's own stream, so work the caller enqueues on ANY of its streams afterwards
 * overlaps it.  Jobs of one context run one after the other in submission order, on a worker thread the context owns -- the tail
 * of an MSM is host arithmetic (window fold, normalisation) and host decisions (out-of-memory back-off, the XYZZ repeat of an
 * Edwards run), which is why completion is a host-side event: `done(user, status)` is called from that thread once
 * `out_projective` (HOST memory, `batches` images) is written -- status.code 0 = success; status.message, if any, is the callback's
 * to free() (SPK util/rusterror.h:15-27) -- and / or the job handle can be polled and waited for.  At least one of `done` and `job`
 * must be given.  mi355_msm_job_wait blocks until the job has finished, returns its status and RELEASES the handle (call it
 * exactly once per handle); mi355_msm_job_done polls (1 = finished).  The synchronous entry points of the same context must not be
 * called while jobs are pending (query "async_pending"); mi355_msm_destroy runs pending jobs to completion first. */
typedef struct mi355_msm_job mi355_msm_job;
typedef void (*mi355_msm_done_fn)(void* user, RustError status);
RustError mi355_msm_run_async(mi355_msm_ctx* ctx, void* out_projective, const void* d_scalars, size_t npoints, size_t batches,
                              void* stream, mi355_msm_done_fn done, void* user, mi355_msm_job** job);
int mi355_msm_job_done(mi355_msm_job* job);
RustError mi355_msm_job_wait(mi355_msm_job* job);

/* "precompute" = 2 (auto, set BEFORE set_bases): the context picks the table levels itself from the device memory that is free at
 * set_bases -- a level per window, else 6, 4 or 3 levels (the shapes profiles/r04_table_levels_sweep.txt shows as wins: -6 % / -3 % /
 * -1.4 % / -1 % at 2^26 pairs), each only if it fits with its build temporaries and leaves the work buffers of a full chunk plus a
 * tenth of the device to the caller; between 2^18 pairs and 2^20 (BLS12-377 G1), 2^19 (BLS12-381 G1), 2^21 (G2) six levels, where
 * they are worth 6 - 23 % (profiles/r06_size_sweep_tables.txt); none at the sizes in between, below 2^18, or when memory is short
 * (about 64 GB free at 2^26), and a build that
 * fails all the same leaves the context on the table-free path.  mi355_msm_query "table_levels" says what it chose.  The harness
 * shims take it from the environment: MI355_MSM_PRECOMPUTE=auto|0|1 (the reference's init builds its tables untimed,
 * CMB MSM.cu:380-383).
 * "precompute" = 1 (set BEFORE set_bases) makes the context store the tables 2^(c w) * P_i for every window w, so all digits
 * of a scalar share one bucket set and the bucket->window reduction and the window fold shrink by the number of windows --
 * the fixed-base trick of the ZPrize winners (CMB PrecomputePoints.cu:10-39; P1A matter-labs/src/lib.rs:101-114), paid for in
 * the untimed init and in HBM (windows x 128 B per base: 94 GB at 2^26, 151 GB with the Edwards records).  Results are identical.
 * "table_levels" = k (with "precompute", BEFORE set_bases; default 0 = a level per window) builds only k levels 2^(c G j) * P_i,
 * j < k, for G = ceil(windows / k) bucket sets: window g + G j reads level j into bucket set g -- the reference's own shape is
 * k = 6 levels and 2 bucket sets for its 23-bit windows (CMB PrecomputePoints.cu:10-39, MSM.cu:380-383).  k times the base memory
 * instead of `windows` times; measured at 2^26 (profiles/r04_table_levels_sweep.txt): all levels 101 ms / 151 GB, k = 6 105 ms /
 * 86 GB, k = 3 107 ms / 47 GB, no tables 108 ms / 21.5 GB.
 * Tuning knobs ("window_bits" 2..24, "lane_entries", "max_chunk" <= 2^27, "seg_entries" >= 4, "reduce_log_chunk" /
 * "reduce_log_chunk0" 1..7: bucket-reduction chunk sizes on all / the first level); 0 restores the automatic choice.
 * ("lane_entries" = 0: 2^20 lanes up to 2^25 pairs, then ~512 entries per lane -- fitted so that the working blocks of the accumulate
 * launch fill their last generation of 256 blocks, one per CU: the launch takes ceil(blocks / 256) generations, profiles/r06_ab_lane_groups.txt.)
 * "reduce_scan" = 0 keeps the bucket reduction on the recursive chunked scheme only (default: its tail is a parallel scan);
 * "reduce_scan_log" 6..18 = log2 of the elements per window at which the scan takes over (default 12).
 * "quad_limit" (per context, default 2^18): merge / scan launches of at most that many additions spread each
 * addition over four lanes (latency); 0 = always one lane per addition.
 * "g2_paired" (G2 contexts; bit mask, default 31 = all; ignored on G1): which throughput kernels hold every Fp2 value on TWO
 * neighbouring lanes (c0 on the even, c1 on the odd one; csrc/fp2pair.hpp) and so run two waves per SIMD instead of one --
 * bit 0 bucket accumulation, 1 first level of the bucket reduction, 2 fragment merge, 3 scan steps, 4 bucket merge of carried
 * batches.  Same records in memory, same result bytes; 0 restores the one-lane-per-point kernels (the A/B of
 * profiles/r05_ab_g2_paired.txt: 2^24 pairs 122 -> 109 ms).
 * "reduce_fill" 1..4 (default 1): waves per SIMD the first chunked level of the bucket reduction is cut for (measured: 2 does
 * not pay, profiles/r05_ab_reduce_fill.txt).
 * "assume_subgroup" = 1 (default 0): the caller guarantees that every base lies in the order-r subgroup (r P = O), as the ZPrize
 * generator's do.  A scalar k in (r/2, r) then runs as (r - k)(-P): the winners' top-bit trick (CMB ProcessSignedDigits.cu:10-20,
 * 123-128), one significant bit less, so BLS12-377 scalars tile 12 windows of 21 bits and the auto window size moves from 20 to 21
 * at 2^26 pairs (-5 % additions; below 2^25 pairs the window choice is left alone).  Off by default because arkworks' msm is exact for ANY curve point and this is not.
 * "anchor" (default 1; 0 off; 2 = always, a test setting): the anchored window.  Signed digits carry, so where the window size leaves
 * (almost) no scalar bits above the last full window -- BLS12-377: 253 = 11 x 23, 252 = 12 x 21 -- the window above it is still
 * non-zero for 14-57 % of the scalars.  assume_subgroup removes those additions by an assumption; this removes them by arithmetic:
 * the carry chain ENDS at the last full window (its value v in [0, 2^c] is taken as 2^(c-1) + s, |s| <= 2^(c-1): the same buckets)
 * and the constant part, 2^(c a + c - 1) x (the plain sum of the bases of the run), is added on the host.  That sum is computed by
 * the library itself (k_sum_bases + the fragment merge: ~n mixed additions, 8 ms at 2^26) in set_bases for runs over all the bases, on
 * the first run of any other length, and kept until the next set_bases.  Exact for ANY input (tests/test_gpu_anchor.py: non-canonical scalars, points outside the subgroup).
 * Used for batches of >= 2^20 pairs, with "carry" on and "assume_subgroup" off, at the window sizes where it saves >= 1 % of the
 * additions; 2^26 pairs of BLS12-377 G1 then run at c = 21 instead of 20 (-1.0 %; with tables -1..-2.5 %: profiles/r06_ab_anchor.txt).
 * The price: a scalar of ZERO costs one addition (its digit in the anchored window is -2^(c-1)) instead of none -- a batch that is
 * mostly zeros should set "anchor" = 0.  The stateless call never uses it (its bases change with every call).
 * "anchor_wide" (default 1; 0 = the recoding above as it is): where exactly ONE bit of r lies above the anchored window a -- BLS12-377's
 * Fr wherever c divides 252: c = 21 at 2^26 pairs; never BLS12-381's -- that bit rides in window a.  Its value v in [0, 2^(c+1)] is taken
 * as 2^c + s, |s| <= 2^c; magnitudes up to 2^(c-1) keep their buckets, the larger ones use the bucket set of the one-bit window above, which
 * has no entries of its own any more: 12.0 n additions instead of 12.14 n at c = 21, the same bucket sets and kernels.  The host adds
 * 2^(c-1) times that set's plain sum (one more row of the bucket reduction) and 2^(c a + c) times the sum of the bases.  -1.3 % at 2^26
 * pairs of BLS12-377 G1, -1.8 % of G2 (profiles/ab_anchor_wide.txt).  A scalar with a bit at or above bits(r) = 253 set is not read
 * that far: the device reports it and the chunk -- of a carried batch: the batch -- runs again without the option, so any 256-bit scalar
 * stays legal; after two such repeats in a row the context stops using it until the option is set again.
 * "entries32" (default 1; 0 = (value, key) pairs of 8 bytes): the last grouping pass writes the sorted entries as one 32-bit word each --
 * base index, sign, and in five spare bits the step of the bucket key from the entry before -- with the key itself stored only where a
 * reader cannot derive it (gaps of more than 30 buckets, the first run of a grouping segment, the start of every accumulation lane).
 * Half the bytes written by the last pass and read by the accumulation: -1.5 % at 2^26 pairs of BLS12-377 G1, -0.9 % of BLS12-381 G1
 * (profiles/ab_entries32.txt).  Applies to chunks of at most 2^26 pairs whose base indices lie below 2^26, without precomputed tables;
 * every other chunk keeps the 64-bit format through the same kernels.  Results never depend on it.
 * "carry" (default 1): a batch that runs as several chunks (max_chunk, the memory budget, the pieces of a host-scalar batch) carries
 * ONE bucket array through them -- every chunk uses the window size of the whole batch and only the last one reduces; 0 = every
 * chunk reduces its own buckets and the partial sums are added on the host.  "first_piece_div" (default 13; 4 with carry = 0): the
 * first batch of a host-scalar run is handed over as pieces of n/div, 3n/div, 9n/div ... each computed while the next crosses PCIe
 * (CMB MSM.cu:419-434 splits its first copy 1/4 + 3/4).
 * Test hooks: "mem_limit" (bytes of device memory chunks may be planned against), "inject_alloc_failures" (N > 0: the next N
 * work-buffer reservations fail; -K: only the K-th from now).
 * "scalars_montgomery" = 1 makes every run treat the scalars as arkworks `Fr` values (Montgomery form, a*2^256 mod r)
 * and convert them on the device first -- VariableBaseMSM::msm(bases, &[Fr]) = into_bigint + msm_bigint
 * (ARK ec/src/msm/variable_base/mod.rs:48-53; sppark's `mont` flag SPK msm/pippenger.cuh:157-164).
 * "scalars_to_montgomery" = 1 is the mirror image: every 256-bit scalar a (any value, not only a < r) runs as a*2^256 mod r, the
 * Montgomery image of a.  That is what the ZPrize harness computes for a data set loaded from TEST_LOAD_DATA_FROM: scalars.bin
 * holds normal-form integers (serialize_unchecked writes into_repr()), the harness deserializes them into `Fr` and hands the MSM
 * the `Fr` limbs through transmute::<&[Fr], &[BigInteger256]> (P1B test_fpga_harness/src/util.rs:72-140, tests/msm.rs:17-40), so
 * arkworks_results.bin[b] = sum (a_i*2^256 mod r) P_i.  Setting both options is an error (-1); 0 turns either off.
 * Mirrors Matter Labs' runtime msm_configuration (P1A matter-labs/.../bellman-cuda.h:49-71). */
RustError mi355_msm_set_option(mi355_msm_ctx* ctx, const char* key, long value);
/* "twisted_edwards" (default 1; set BEFORE set_bases; BLS12-377 G1 only) lets the context keep, next to the bases, their image on
 * the birationally equivalent twisted Edwards curve -X^2 + Y^2 = 1 + d X^2 Y^2 and accumulate there: 7 field multiplications
 * per mixed addition instead of 8M + 2S, no doubling/infinity branches (the trick of P1A Trapdoor-Tech/msm_opt.md and of the FPGA
 * entries).  Results are identical BY CONSTRUCTION, not by assumption: a base set containing one of the five points without
 * an image (e.g. the FPGA harness's 2-torsion fixture) stays on the short-Weierstrass path, and because d is a square the
 * kernels check every addition for a vanishing denominator (possible only for inputs outside the prime-order subgroup) and
 * the run is then repeated on the short-Weierstrass path.  Costs 192 B per base (per table level) of HBM on top. */
/* State of a context: "twisted_edwards" (1 = the current bases run on the twisted-Edwards path), "twisted_edwards_fallbacks"
 * (chunks repeated on the XYZZ path so far), "twisted_edwards_demotions" (two fallbacks in a row demote the base set to XYZZ
 * until the next set_bases), "oom_backoffs" (chunks restarted at half size after a device allocation failed -- after the idle
 * contexts of the stateless pool were given back and the same chunk retried), "debug_checks" (invariant checks a -DMSM_DEBUG
 * build has run; always 0 in this library), "chunk_cap", "anchor" (the option), "anchored_window" (1 + the anchored window of the most
 * recent chunk, 0 = plain digits), "anchor_sums" (sums of bases computed so far), "anchor_sum_us" (host time the most recent run spent on one),
 * "anchor_wide" (the option; 0 once the context has stopped using it), "anchor_wide_active" (the most recent chunk ran with it),
 * "anchor_wide_fallbacks" (chunks / batches repeated without it), "anchor_wide_demotions",
 * "entries32" (the option), "entries32_active" (the most recent chunk's sorted entries were 32-bit words),
 * "reduce_path" (how the most recent chunk's buckets were reduced: 0 recursive chunked levels only, 1 direct scan on the buckets, 2 one
 * chunked level then a scan on full rows, 3 the same on rows padded to a power of two), "reduce_chunks" (chunks per bucket set on the
 * first level) and "reduce_row" (elements of a scan row),
 * "device", "bases", "table_levels", "table_window_bits", "base_bytes" (device bytes held for the bases). */
RustError mi355_msm_query(mi355_msm_ctx* ctx, const char* key, uint64_t* value);
/* Per-stage device time (ms, HIP events on the launch stream) of the most recent run, summed over its chunks
 * and batches (MI355_T_HOST_FOLD: host wall time of the final normalisation); ms must hold MI355_T_COUNT floats.
 * info (8 words): [0]=window bits, [1]=windows, [2]=sorted entries of the last chunk, [3]=entries per lane, [4]=accumulate
 * launches, [5]=lanes of the last launch, [6]=1 when precomputed tables were used, [7]=1 on the twisted-Edwards path.
 * Chunks are sized to the device memory that is free (the reference plans its allocations first, ML msm.cu:453-466), and a
 * chunk whose allocation fails all the same is retried at half the size. */
RustError mi355_msm_last_timings(mi355_msm_ctx* ctx, float* ms, uint64_t* info);
/* The same for ONE shard of a sharded context (mi355_msm_last_timings reports the slowest shard per stage): an imbalance
 * between the devices shows here.  shard 0 of an ordinary context is the context itself. */
RustError mi355_msm_shard_timings(mi355_msm_ctx* ctx, int shard, float* ms, uint64_t* info);

/* ---- stateless calls ---------------------------------------------------------------------------
 * sppark's mult_pippenger_inf(out, points, npoints, scalars, ffi_affine_sz)
 * (SPK poc/blst-cuda/cuda/pippenger_inf.cu:28-35) with the curve made explicit; BASELINE.json's
 * `msm(bases, scalars, n)` is mi355_msm(curve, out, bases, n, scalars, 104). */
RustError mi355_msm(int curve, void* out_projective, const void* affine, size_t npoints, const void* scalars,
                    size_t ffi_affine_sz);
/* The call is a pipeline, as in the reference (SPK msm/pippenger.cuh:617-661 uploads the next slice of points and scalars
 * while the current one is sorted and accumulated; CMB MSM.cu:419-434; the growing chunks of P1A matter-labs/src/lib.rs:171-182):
 * slices of 2^20..2^23 pairs are staged by a few host threads through a small ring of pinned buffers (kept for the life of the
 * process; mi355_msm_trim() gives it back) and cross PCIe while earlier slices are converted and run; partial sums are added
 * on the host.  Environment: MI355_MSM_STAGE_THREADS (default 6), MI355_MSM_STATELESS_SLICE_LOG (log2 pairs per slice),
 * MI355_MSM_STATELESS_RAMP (default 1: the first two slices are 1/8 and 1/2 of a slice; 0: one half slice first).
 * With MI355_MSM_DEVICES naming several GPUs every shard runs its own pipeline over its slice of both operands.
 * mi355_msm_last_stateless: what the calling thread's most recent stateless call did -- out[0..7] = total ms, setup ms (buffers,
 * ring, threads), ms the compute side waited for uploads, ms it spent issuing/awaiting slices, the last slice's share of that
 * (the tail nothing overlaps), slices, staging threads, bytes moved; out[8] = ms from the start of the call to the completion of its LAST
 * DMA (total ms - out[8] is what the call spends after the uploads are over: the bound is PCIe when that is one slice's compute,
 * the device when it is more), out[9] = ms at which the copy stream started. */
RustError mi355_msm_last_stateless(double* out, size_t count);
/* What the stateless entry points keep between calls, and its bounds: the pinned staging rings (12 x 16 MiB per device in use) and at
 * most ONE idle context per (curve, device) with its device buffers (~9 GB after a 2^26-pair G1 call; a context above
 * MI355_MSM_STATELESS_KEEP_MB, default 16384, is parked without its buffers).  Any device allocation of this library that runs out
 * of memory frees the idle contexts and retries before it fails.  mi355_msm_trim() frees rings and idle contexts now;
 * mi355_msm_pool_stats: out[0] = idle contexts, out[1] = device bytes they hold, out[2] = idle rings, out[3] = pinned bytes they hold. */
RustError mi355_msm_trim(void);
RustError mi355_msm_pool_stats(uint64_t* out, size_t count);

/* ---- arkworks' streaming accumulators (ARK ec/src/msm/variable_base/stream_pippenger.rs) ---------------------------------
 * ChunkedPippenger::{new, with_size, add, finalize} (:11-75) and HashMapPippenger::{new, add, finalize} (:78-140): what a prover
 * holds across rounds.  `hashmap` = 0: buffer pairs, and whenever the buffer holds max_msm_buffer of them, result += MSM(buffer).
 * `hashmap` = 1: a pair whose base (x, y, infinity flag) is already buffered adds its scalar to that entry modulo the scalar
 * field order r -- scalars are Fr values there -- and the MSM runs when max_msm_buffer DISTINCT bases are buffered.
 * add() takes `count` pairs (bases `stride` bytes apart) and behaves exactly like `count` single adds.  finalize() flushes what
 * is left, writes the normalised Projective image and leaves the accumulator empty for reuse (arkworks' finalize consumes it).
 * Each flush is the stateless pipeline of mi355_msm() on `device` (< 0: the current device).  Options: "scalars_montgomery"
 * (the scalars are arkworks Fr images, converted on the device -- sums of Montgomery images are Montgomery images of sums),
 * "scalars_to_montgomery" (each scalar a runs as a*2^256 mod r, see mi355_msm_set_option), "window_bits".  Queries: "buffered", "flushes", "merged" (pairs that landed on an existing hashmap entry), "buf_size". */
typedef struct mi355_msm_stream mi355_msm_stream;
RustError mi355_msm_stream_create(mi355_msm_stream** out, int curve, int device, size_t max_msm_buffer, int hashmap);
RustError mi355_msm_stream_set_option(mi355_msm_stream* s, const char* key, long value);
RustError mi355_msm_stream_add(mi355_msm_stream* s, const void* affine, size_t stride, const void* scalars, size_t count);
RustError mi355_msm_stream_finalize(mi355_msm_stream* s, void* out_projective);
RustError mi355_msm_stream_query(mi355_msm_stream* s, const char* key, uint64_t* value);
RustError mi355_msm_stream_destroy(mi355_msm_stream* s);

/* ---- batch fixed-base scalar multiplication (ARK ec/src/msm/fixed_base.rs:8-97) ------------------------------------------------
 * out[i] = s_i * g for ONE base g and n scalars: FixedBase::{get_mul_window_size, get_window_table, windowed_mul, msm} followed by
 * batch_normalization_into_affine -- what a KZG / Groth16 setup runs for [tau^i] G, and what produces the bases an MSM consumes.
 * A handle is the window table of one base, resident on one device: level j holds d * 2^(w j) * g for every w-bit digit d
 * (ceil(256 / w) levels, unsigned digits), built on the device by mi355_msm_fixed_create.
 *   g        one arkworks Affine image (104 B / 200 B; only the bytes up to the flag byte are read; the flag byte is authoritative).
 *            ANY curve point: off the subgroup, of small order, or flagged infinity (every output is then infinity).
 *   scalars  32 B little-endian integers; ALL 256 bits count -- the result is the integer multiple, never reduced modulo r, because g
 *            need not have order r.  Flag bit 0: the 32 B are arkworks Fr images (a * 2^256 mod r) and are converted first
 *            (FixedBase::msm takes &[ScalarField] and calls into_bigint, fixed_base.rs:66-67); defined for any 256-bit image.
 *   out      one image per scalar, in input order, out_stride bytes apart (a multiple of 4, at least the image size; bytes between
 *            two images are not written).  Default: arkworks Affine images -- x, y canonical, flag byte 0, pad bytes 0; the point at
 *            infinity is all zeros with flag 1 (arkworks 0.4) -- ready for mi355_msm_set_bases[_device] and mi355_msm_check_bases.
 *            Flag bit 1: normalised Projective images, byte for byte what mi355_msm_run writes for the one-pair MSM (g, s_i).
 * Results never depend on the window size, on chunking, or on host versus device pointers.
 * window_bits 1..20, 0 = automatic from expected_scalars (0 = unknown: plan for a large batch): the cheapest of
 * levels(w) * (2 * 2^w + expected_scalars) additions with the table inside the Infinity Cache (at most 16 bits for G1: 134 MB, 15 for
 * G2: 151 MB).  mi355_msm_fixed_window_size is arkworks' own rule -- 3 below 32 scalars, else ceil(log2 n) * 69 / 100 -- exported for
 * API parity only: it is a CPU cache heuristic and no handle uses it.
 * mi355_msm_fixed_mul takes HOST pointers, mi355_msm_fixed_mul_device DEVICE pointers (4-byte aligned) and the hipStream_t on which
 * the scalars become ready (NULL = the default stream); its work is enqueued there and the call returns when the output is written.
 * n = 0 is a success that writes nothing.  Work memory does not grow with n: calls run in chunks of "max_chunk" scalars
 * (mi355_msm_fixed_set_option, default 2^22, 0 restores it; a test hook -- results do not depend on it).
 * Queries: "window_bits", "levels", "table_bytes", "signed_digits" (0), "build_us" (host clock around the table build), "device",
 * "last_mul_us" (host clock around the most recent call), "last_device_us" (the same call between events on the stream it ran on),
 * "max_chunk", "work_bytes" (chunk buffers held).
 * Errors: -1 with a message for null pointers, a stride too small or not a multiple of 4, an unknown curve, window_bits outside 0..20,
 * unknown flag bits -- decided before any device call; hipErrorNoDevice without a GPU. */
typedef struct mi355_msm_fixed mi355_msm_fixed;
size_t mi355_msm_fixed_window_size(size_t num_scalars);
RustError mi355_msm_fixed_create(mi355_msm_fixed** out, int curve, int device, const void* base_affine, int window_bits, size_t expected_scalars);
RustError mi355_msm_fixed_mul(mi355_msm_fixed* fb, void* out, size_t out_stride, const void* scalars, size_t n, unsigned flags);
RustError mi355_msm_fixed_mul_device(mi355_msm_fixed* fb, void* d_out, size_t out_stride, const void* d_scalars, size_t n, unsigned flags,
                                     void* stream);
RustError mi355_msm_fixed_set_option(mi355_msm_fixed* fb, const char* key, long value);
RustError mi355_msm_fixed_query(mi355_msm_fixed* fb, const char* key, uint64_t* value);
RustError mi355_msm_fixed_destroy(mi355_msm_fixed* fb);

/* ---- batch variable-base scalar multiplication (ARK ec/src/lib.rs:188,294,305-319, models/short_weierstrass.rs:413-422) ----------
 * out[i] = s_i * P_i: AffineRepr::mul_bigint / mul_by_cofactor over a whole vector, followed by batch_normalization_into_affine --
 * what a ceremony contribution runs over the previous transcript, and the second half of drawing random subgroup points (solve for y,
 * then multiply by the cofactor).  The calls sit on a single-device context (a sharded one refuses them with -1).
 *   points   arkworks Affine images, `stride` bytes apart (a multiple of 4, at least 2 coordinates + the flag byte), read exactly as
 *            mi355_msm_set_bases reads them.  The flag byte is authoritative (a flagged infinity may carry junk coordinates).  The
 *            point may be off the subgroup or of small order: there is no curve test and no subgroup test, as mul_bigint has none.  A
 *            record that is on no curve gives an unspecified result; the call still finishes without a fault.
 *   scalars  default (pairwise): npoints x 32 B little-endian integers, scalar_bytes = 32.  ALL 256 bits count -- the result is the
 *            integer multiple, never reduced modulo r (the fixed-base contract, for the same reason).  Flag bit 0: the 32 B are
 *            arkworks Fr images (a * 2^256 mod r) and are converted first; defined for any 256-bit image.
 *            Flag bit 2, one scalar for all points: `scalars` is a HOST pointer (also in the _device call) to ONE little-endian
 *            integer of scalar_bytes bytes, a multiple of 4 from 4 to 64 (the G2 cofactors are 502 and 507 bits long).  Bit 0 is
 *            refused together with bit 2.
 *            Flag bit 3 (implies bit 2): the scalar is the curve's COFACTOR -- arkworks' mul_by_cofactor; `scalars` must be NULL and
 *            scalar_bytes 0.  This is NOT clear_cofactor, which for BLS12-381 is a different map with a different result.
 *   out      one image per point, in input order, out_stride bytes apart (a multiple of 4, at least the image size; bytes between two
 *            images are not written).  Default: arkworks Affine images -- x, y canonical, every flag and pad byte written, infinity all
 *            zeros with flag 1.  Flag bit 1: normalised Projective images, byte for byte what mi355_msm_run writes for the one-pair
 *            MSM (P_i, s_i).  `out` must NOT overlap `points`.
 * Pairwise: per point a table 1P .. 2^(w-1) P, normalised, then ceil(257 / w) signed w-bit digits from the top (w doublings and one
 * mixed addition each), starting at the highest window that is non-zero in any of the 64 points of a wave.  One scalar: its
 * non-adjacent form, one doubling per digit and one mixed addition per non-zero digit, no table.
 * Results never depend on chunking, on the window size, or on host versus device pointers.  npoints = 0 succeeds and writes nothing.
 * Work memory does not grow with npoints: calls run in chunks through buffers the context keeps until it is destroyed.  Options
 * (mi355_msm_set_option): "mul_chunk", points per chunk (0 restores the default: the largest power of two whose work buffers stay
 * within 2 GiB -- 2^19 for G1, 2^18 for G2; a wider window lowers it), "mul_window" 1..6 (0 restores the default, 4; a test hook).
 * Queries: "mul_window", "mul_chunk", "mul_work_bytes" (chunk buffers held), "last_mul_us" (host clock around the most recent call),
 * "last_mul_device_us" (the same call between events on the stream it ran on).
 * mi355_msm_mul_points takes HOST pointers; mi355_msm_mul_points_device DEVICE pointers (4-byte aligned) for points, pairwise scalars
 * and out, and the hipStream_t on which they become ready (NULL = the default stream): its work is enqueued there and the call returns
 * when the output is written.
 * Errors: -1 with a message for null pointers, a stride too small or not a multiple of 4, a scalar_bytes value the mode does not allow,
 * unknown or contradictory flag bits -- decided before any device call; hipErrorNoDevice without a GPU. */
RustError mi355_msm_mul_points(mi355_msm_ctx* ctx, const void* points, size_t npoints, size_t stride, const void* scalars, size_t scalar_bytes,
                               unsigned flags, void* out, size_t out_stride);
RustError mi355_msm_mul_points_device(mi355_msm_ctx* ctx, const void* d_points, size_t npoints, size_t stride, const void* scalars,
                                      size_t scalar_bytes, unsigned flags, void* d_out, size_t out_stride, void* stream);

/* ---- radix-2 evaluation domains over the scalar fields (ARK poly/src/domain/radix2/mod.rs, domain/mod.rs:78-170, :233) ------------
 * Radix2EvaluationDomain::{fft, ifft, coset_fft, coset_ifft} and the pointwise product, on the device: the step before the MSM in a
 * prover (evaluations -> ifft -> commit).  The output of a transform in device memory is what mi355_msm_run_device reads under the
 * option "scalars_montgomery", so nothing crosses PCIe between the two.
 * A handle is ONE domain size n = 2^k on one device.  Any of the four curve ids selects its family's Fr (BLS12-377: 253 bits, 2-adicity
 * 47; BLS12-381: 255 bits, 2-adicity 32).  num_coeffs is rounded up to a power of two, as Radix2EvaluationDomain::new does; the call
 * fails with -1 above the field's 2-adicity and above 2^28.  omega = get_root_of_unity(n): TWO_ADIC_ROOT_OF_UNITY squared s - k times.
 *   kind     0 forward    out[i] = sum_{j<n} in[j] * omega^(i j)
 *            1 inverse    out[j] = n^-1 * sum_{i<n} in[i] * omega^(-i j)
 *            2 coset forward   out[i] = sum_j in[j] * (g omega^i)^j            (distribute_powers, then forward)
 *            3 coset inverse   out[j] = g^-j * n^-1 * sum_i in[i] * omega^(-i j)   (inverse, then distribute_powers_and_mul_by_const)
 *   offset   g: a HOST pointer (also in the _device call) to one 32-byte element in the form of the call; NULL = GENERATOR (22 / 7).
 *            Kinds 2 and 3 only; zero is refused.  The handle keeps the tables of the most recent offset.
 *   elements 32 bytes.  Default: arkworks Fr images (a * 2^256 mod r, what a Vec<Fr> holds).  Flag bit 0: plain little-endian
 *            integers on both sides.  ANY 256-bit input is read as its residue modulo r; every output is canonical (< r).
 *   in_len   <= n; elements from in_len on (in the order they are stored) are read as zero and never touched -- arkworks' resize in
 *            fft_in_place.  in_len > n is an error, not a truncation.  in may be NULL when in_len is 0.
 *   batch    vectors, n elements apart in both `in` and `out` (the reference's NTT_batch); at most 65535.  batch = 0 succeeds and
 *            writes nothing.
 *   order    natural in, natural out by default.  Flag bit 1 (kinds 0, 2): the output in bit-reversed order; flag bit 2 (kinds 1, 3):
 *            the input in bit-reversed order -- the pair round a pointwise step.
 *   out == in is allowed; any other overlap of the bytes read (up to element in_len of the last vector) with the bytes written
 *            (batch whole vectors) is an error.
 * A transform is ceil(k / pass_log) launches.  Each is one Stockham pass that reads and writes natural order, so no launch permutes;
 * a block takes 1024 points through up to 10 butterfly levels in LDS.  The powers of g, the factor n^-1 and the conversions of the
 * element form are folded into the first load and the last store.  Twiddles come from two-level tables (omega^lo, omega^(hi 2^14)),
 * built on the device by mi355_msm_domain_create: 3.6 MB at k = 28.
 * Work memory: one vector per vector in flight (batch * n * 32 bytes), kept by the handle; a host-pointer call stages one vector at a
 * time through one more.  A handle serves one call at a time.
 * mi355_msm_domain_mul: out[i] = a[i] * b[i] over n elements (any n; mul_polynomials_in_evaluation_domain), flag bit 0 as above; out may
 * be a or b.
 * mi355_msm_domain_element: omega^i as an arkworks image (host arithmetic).
 * The calls without _device take HOST pointers; the _device calls DEVICE pointers (4-byte aligned) and the hipStream_t on which the
 * input becomes ready (NULL = the default stream): the work is enqueued there and the call returns when the output is written.
 * Option "pass_log" 1..10 (0 restores the default, 8): butterfly levels per pass -- a test hook.  Results never depend on it, nor on
 * host versus device pointers, nor on batching.
 * Queries: "size", "log_size", "passes", "pass_log", "table_bytes", "work_bytes", "poly_work_bytes", "scan_work_bytes", "quotient_work_bytes", "poly_tile_log", "device", "last_us" (host clock around the most recent
 * call), "last_device_us" (the same call between events on the stream it ran on).
 * Errors: -1 with a message for null pointers, in_len > n, a partial overlap, unknown or misplaced flag bits, an unknown kind, an offset
 * on a plain transform, a size above the limits -- decided before any device call; hipErrorNoDevice without a GPU. */
typedef struct mi355_msm_domain mi355_msm_domain;
RustError mi355_msm_domain_create(mi355_msm_domain** out, int curve, int device, size_t num_coeffs);
RustError mi355_msm_domain_transform(mi355_msm_domain* d, void* out, const void* in, size_t in_len, size_t batch, unsigned kind, unsigned flags,
                                     const void* offset);
RustError mi355_msm_domain_transform_device(mi355_msm_domain* d, void* d_out, const void* d_in, size_t in_len, size_t batch, unsigned kind,
                                            unsigned flags, const void* offset, void* stream);
RustError mi355_msm_domain_mul(mi355_msm_domain* d, void* out, const void* a, const void* b, size_t n, unsigned flags);
RustError mi355_msm_domain_mul_device(mi355_msm_domain* d, void* d_out, const void* d_a, const void* d_b, size_t n, unsigned flags, void* stream);
RustError mi355_msm_domain_set_option(mi355_msm_domain* d, const char* key, long value);
RustError mi355_msm_domain_query(mi355_msm_domain* d, const char* key, uint64_t* value);
RustError mi355_msm_domain_element(mi355_msm_domain* d, uint64_t i, void* out32);
RustError mi355_msm_domain_destroy(mi355_msm_domain* d);

/* ---- between a transform and an MSM: batch inversion, evaluation, division by X - z, Lagrange coefficients, element-wise calls ---------
 * (ARK ff/src/fields/mod.rs:811-873 batch_inversion_and_mul; poly/src/polynomial/univariate/dense.rs:41-94 evaluate;
 * poly/src/polynomial/univariate/mod.rs:102 divide_with_q_and_r by X - z; poly/src/domain/radix2/mod.rs:141-216
 * evaluate_all_lagrange_coefficients, evaluate_vanishing_polynomial; poly/src/domain/mod.rs:190-197
 * divide_by_vanishing_poly_on_coset_in_place.)  With them the Groth16 / Marlin quotient
 * h = coset_ifft((coset_fft(a) * coset_fft(b) - coset_fft(c)) / Z(g)) and a KZG opening (p(z), (p - p(z)) / (X - z), then the MSM of
 * the quotient) run from coefficients to commitment in device memory.
 * All of them live on the domain handle and follow its conventions: 32-byte elements, arkworks Fr images or, with flag bit 0 (the only
 * flag), plain integers; ANY 256-bit input is read as its residue and every output is canonical; the calls without _device take HOST
 * pointers and stage whole vectors through buffers the handle keeps, the _device calls take DEVICE pointers (4-byte aligned) and the
 * stream on which the input becomes ready, and return when the output is written.  The scalars z, tau, coeff, offset and the factor
 * of the scaling are ONE HOST element in the form of the call, also in the _device calls, and so are the results out32 / rem32.
 * Vector lengths are any n up to 2^30 and have nothing to do with the domain's size, except for the Lagrange call.
 *   batch_inverse   out[i] = coeff / in[i]; coeff NULL = 1.  An element that is 0 modulo r (the byte patterns r, 2r, .. included)
 *                   gives canonical 0, as arkworks skips zeros.  out == in is allowed; any other overlap is refused.
 *   vec_op          op 0: a + b;  1: a - b;  2: a * b - c;  3: s * a, where b points to the one HOST element s.  c is read by op 2
 *                   only.  out may be any of the input vectors exactly; a partial overlap is refused.  (mi355_msm_domain_mul stays.)
 *   evaluate        out32 = sum_i coeffs[i] z^i.  n = 0 gives 0; z = 0 gives coeffs[0].
 *   divide_by_linear  q_out[i] = sum_(j > i) coeffs[j] z^(j - i - 1) for i < n - 1: the n - 1 coefficients of (p - p(z)) / (X - z),
 *                   leading zeros kept; rem32 = p(z) (may be NULL).  Any overlap of q_out with coeffs is refused.  n <= 1 writes no
 *                   quotient (q_out may be NULL).
 *   lagrange        the `size` values L_i(tau) = Z(tau) omega^i / (size (tau - omega^i)); tau in the domain gives the unit vector.
 *   vanishing       out32 = tau^size - 1, in host arithmetic like mi355_msm_domain_element.
 *   divide_by_vanishing_on_coset  out[i] = in[i] / (g^size - 1) for the coset offset g (NULL = GENERATOR): the scaling with a factor
 *                   derived on the host.  out == in is allowed.  An offset that is zero or lies in the domain (Z(g) = 0) is an error.
 * The three scans share one tiled scheme (csrc/poly.hpp): a block takes a tile of 1024 consecutive elements through LDS, 256 lanes own 4
 * neighbours each.  The inversion is three launches: the product of every tile; one Fermat inversion per TILE, one lane each; then
 * Montgomery's trick inside the tile.  The evaluation reduces every tile to one partial and runs again on the partials; the division
 * is that way up, then a way down on which every tile is read again with the carry that enters it.  Levels are separate launches on
 * one stream: no block waits on another, nothing is atomic.  Work memory: the partials and carries, 2 (n / 1024 + n / 1024^2 + ..)
 * elements of 36 bytes, allocated on the first such call and kept by the handle, plus the staged vectors of host-pointer calls --
 * query "poly_work_bytes" ("work_bytes" keeps its meaning).  Option "poly_tile_log" 4..10 (0 restores the default, 10): a test hook,
 * results never depend on it; also a query.
 * Errors: -1 with a message for null pointers, a partial overlap, unknown flag bits, an unknown op, n above 2^30, a bad offset and, last,
 * a null handle -- decided before any device call; hipErrorNoDevice without a GPU (no handle can be created). */
RustError mi355_msm_domain_batch_inverse(mi355_msm_domain* d, void* out, const void* in, size_t n, const void* coeff, unsigned flags);
RustError mi355_msm_domain_batch_inverse_device(mi355_msm_domain* d, void* d_out, const void* d_in, size_t n, const void* coeff, unsigned flags,
                                                void* stream);
RustError mi355_msm_domain_vec_op(mi355_msm_domain* d, void* out, const void* a, const void* b, const void* c, size_t n, unsigned op, unsigned flags);
RustError mi355_msm_domain_vec_op_device(mi355_msm_domain* d, void* d_out, const void* d_a, const void* d_b, const void* d_c, size_t n, unsigned op,
                                         unsigned flags, void* stream);
RustError mi355_msm_domain_evaluate(mi355_msm_domain* d, void* out32, const void* coeffs, size_t n, const void* z, unsigned flags);
RustError mi355_msm_domain_evaluate_device(mi355_msm_domain* d, void* out32, const void* d_coeffs, size_t n, const void* z, unsigned flags,
                                           void* stream);
RustError mi355_msm_domain_divide_by_linear(mi355_msm_domain* d, void* q_out, void* rem32, const void* coeffs, size_t n, const void* z,
                                            unsigned flags);
RustError mi355_msm_domain_divide_by_linear_device(mi355_msm_domain* d, void* d_q_out, void* rem32, const void* d_coeffs, size_t n, const void* z,
                                                   unsigned flags, void* stream);
RustError mi355_msm_domain_lagrange(mi355_msm_domain* d, void* out, const void* tau, unsigned flags);
RustError mi355_msm_domain_lagrange_device(mi355_msm_domain* d, void* d_out, const void* tau, unsigned flags, void* stream);
RustError mi355_msm_domain_vanishing(mi355_msm_domain* d, void* out32, const void* tau, unsigned flags);
RustError mi355_msm_domain_divide_by_vanishing_on_coset(mi355_msm_domain* d, void* out, const void* in, size_t n, const void* offset,
                                                        unsigned flags);
RustError mi355_msm_domain_divide_by_vanishing_on_coset_device(mi355_msm_domain* d, void* d_out, const void* d_in, size_t n, const void* offset,
                                                               unsigned flags, void* stream);

/* ---- prefix scans along a vector of Fr and the Plonk permutation grand product -----------------------------------------------------------
 * What a Plonk prover's second round needs between the wires and ifft + MSM: z[0] = 1,
 * z[j+1] = z[j] * prod_i (w_i[j] + beta k_i omega^j + gamma) / prod_i (w_i[j] + beta sigma_i[j] + gamma); and, with the sum, the running
 * sum of logUp / lookup arguments.  The calls live on the domain handle and follow the conventions of the calls above: 32-byte
 * elements, arkworks Fr images or, with flag bit 0, plain integers; ANY 256-bit input is read as its residue and every output is
 * canonical; host pointers without _device, device pointers (4-byte aligned) and a stream with it; total32, ks, beta and gamma are HOST
 * elements in the form of the call, also in the _device calls.
 *   scan            op 0: the product (identity 1); op 1: the sum (identity 0).  Exclusive by default: out[0] = identity,
 *                   out[i] = in[0] o .. o in[i-1]; flag bit 1: inclusive, out[i] = in[0] o .. o in[i].  total32 (may be NULL) = the
 *                   combination of all n inputs; n = 0 writes the identity there and nothing else.  n is any length up to 2^30 and has
 *                   nothing to do with the domain's size.  out == in is allowed; any other overlap is refused.
 *                   ZEROS ARE NOT SKIPPED: after an input that is 0 modulo r every later product is 0.  (batch_inverse skips zeros,
 *                   as arkworks does; a scan has no such habit to follow.)
 *   permutation_product  n = the size of the handle.  wires and sigmas hold m columns (1 <= m <= 8) of n elements, `stride` >= n
 *                   elements apart; ks: the m coset representatives.  The identity permutation's value of cell (i, j) is
 *                   ks[i] * omega^j, taken from the handle's tables: no id vector is passed.  With f[j] = the quotient above,
 *                   out[0] = 1, out[j] = prod_(t<j) f[t] (n elements) and total32 (may be NULL) = out[n-1] * f[n-1], which is 1 exactly
 *                   when the copy constraints hold.  out may not overlap the inputs.  Flag bit 0 is the only flag.
 *                   A ZERO DENOMINATOR IS NOT AN ERROR: the batch inversion leaves it zero, so f[j] = 0 and every later out[] and
 *                   total32 are 0.
 * Scheme (csrc/scan.hpp): the tiles of the calls above.  Way up: one total per tile (the lane's run, then a tree); the vector of totals
 * is scanned the same way (three levels at 2^30); way down: every tile is read again, a Hillis-Steele scan runs over its 256 lane
 * totals, the carry that enters the tile is folded in and the tile is stored.  The permutation product is one kernel for the m-fold
 * numerators and denominators, the three launches of the batch inversion on the denominators, and the product scan, whose load
 * multiplies the two.  Levels are separate launches on one stream: no block waits on another, nothing is atomic.
 * Work memory is allocated on the first such call and kept by the handle: query "scan_work_bytes" ("work_bytes" and "poly_work_bytes"
 * keep their meaning and their values).  Results never depend on "poly_tile_log", on host versus device pointers or on `stride`.
 * Errors: -1 with a message for unknown flag bits, n above 2^30, an unknown op, m outside 1..8, null pointers, a partial overlap, a stride
 * of 0 and, last, a null handle -- decided before any device call; a stride below n and an output that overlaps the columns are judged
 * against the handle's size. */
RustError mi355_msm_domain_scan(mi355_msm_domain* d, void* out, void* total32, const void* in, size_t n, unsigned op, unsigned flags);
RustError mi355_msm_domain_scan_device(mi355_msm_domain* d, void* d_out, void* total32, const void* d_in, size_t n, unsigned op, unsigned flags,
                                       void* stream);
RustError mi355_msm_domain_permutation_product(mi355_msm_domain* d, void* out, void* total32, const void* wires, const void* sigmas, size_t m,
                                               size_t stride, const void* ks, const void* beta, const void* gamma, unsigned flags);
RustError mi355_msm_domain_permutation_product_device(mi355_msm_domain* d, void* d_out, void* total32, const void* d_wires, const void* d_sigmas,
                                                      size_t m, size_t stride, const void* ks, const void* beta, const void* gamma, unsigned flags,
                                                      void* stream);

/* ---- the rows of the Plonk quotient and linear combinations of Fr vectors ---------------------------------------------------------------
 * What a TurboPlonk prover's third round needs between its 25 coset_ffts and the coset_ifft (Jellyfish's compute_quotient_polynomial),
 * and the sum sum_j c_j p_j(X) with host scalars of its fourth and fifth (the linearisation and the batched opening polynomial).  The
 * calls live on the domain handle and follow the conventions of the calls above: 32-byte elements, arkworks Fr images or, with flag
 * bit 0 (the only flag), plain integers; ANY 256-bit input is read as its residue and every output is canonical; host pointers without
 * _device, device pointers (4-byte aligned) and a stream with it; ks, alpha, beta, gamma, offset and coeffs are HOST elements in the form
 * of the call, also in the _device calls.
 *   plonk_quotient  the handle is the QUOTIENT domain, of M = 2^K points; n, a power of two, is the size of the constraint domain and
 *                   ratio = M / n is 2, 4, 8 or 16.  Every vector holds M evaluations on offset * H_M in natural order, what the coset
 *                   transform of kind 2 writes (offset NULL: GENERATOR).  wires and sigmas hold m columns `stride` >= M elements
 *                   apart; selectors is NULL or holds 13 columns with the same stride in the order q_lc[0..3], q_mul[0..1],
 *                   q_hash[0..3], q_o, q_c, q_ecc, and then m == 5; with selectors == NULL, 1 <= m <= 8 and the gate term is pi[i]
 *                   alone, for a prover that brings the evaluations of a gate of its own.  z: the permutation polynomial; pi may be
 *                   NULL, meaning 0; ks: m elements.  For row i, with x = offset * omega_M^i:
 *                     t_circ  = q_c + pi + sum_(j<4) q_lc[j] w_j + q_mul[0] w0 w1 + q_mul[1] w2 w3 + q_ecc w0 w1 w2 w3 w4
 *                               + sum_(j<4) q_hash[j] w_j^5 - q_o w4
 *                     t_perm1 = alpha (z[i] prod_j (w_j + beta ks[j] x + gamma) - z[(i + ratio) mod M] prod_j (w_j + beta sigma_j + gamma))
 *                     t_perm2 = alpha^2 (z[i] - 1) / (n (x - 1))
 *                     out[i]  = (t_circ + t_perm1) / ((offset omega_M^(i mod ratio))^n - 1) + t_perm2
 *                   out may not overlap any input: z is read `ratio` rows ahead.  An offset that is 0, or with
 *                   (offset omega_M^i)^n = 1 for some i < ratio, is an error, judged in host arithmetic as
 *                   divide_by_vanishing_on_coset judges its own.  AFTER THAT CHECK x - 1 IS NEVER 0 (an offset inside H_M fails it), so
 *                   the zero convention of the batch inversion underneath cannot be reached.  Sums over several proving instances
 *                   (the reference's alpha_base) stay with vec_op.
 *   linear_combination  cols: a HOST array of m pointers (1 <= m <= 32) to vectors of lens[j] <= 2^30 elements; coeffs: m elements.
 *                   out[i] = sum_j coeffs[j] * cols[j][i] for i < max(lens); a column contributes 0 past its length; max(lens) == 0
 *                   writes nothing.  out may be exactly one of the columns; any other overlap is refused.  The length has nothing
 *                   to do with the domain's size.
 * Scheme (csrc/quotient.hpp): one kernel writes x_i - 1 into work memory, the three launches of the batch inversion turn it into
 * alpha^2 / (n (x_i - 1)) in place, and one kernel with one lane per row and one rolled loop over the columns does the rest; the `ratio`
 * inverses of Z_H, alpha, alpha^2 / n, beta ks[j] and gamma are prepared on the host.  The linear combination is one launch and one
 * pass.  Separate launches on one stream: no block waits on another, nothing is atomic.
 * Work memory is allocated on the first such call and kept by the handle: query "quotient_work_bytes" ("work_bytes", "poly_work_bytes"
 * and "scan_work_bytes" keep their meaning and their values).  Results never depend on "poly_tile_log", on host versus device pointers
 * or on `stride`.  There is no CPU fallback.
 * Errors: -1 with a message for unknown flag bits, m outside its range (5 with selectors, 1..8 without, 1..32 columns of a combination),
 * n not a power of two or too large for any ratio, a stride of 0, a length above 2^30, null pointers, an output that is an input, an
 * offset of 0 and, last, a null handle -- decided before any device call; the ratio, a stride below M, the overlap of whole columns and
 * the offset's residue are judged against the handle. */
RustError mi355_msm_domain_plonk_quotient(mi355_msm_domain* d, void* out, const void* wires, const void* sigmas, const void* selectors, const void* z,
                                          const void* pi, size_t m, size_t stride, size_t n, const void* ks, const void* alpha, const void* beta,
                                          const void* gamma, const void* offset, unsigned flags);
RustError mi355_msm_domain_plonk_quotient_device(mi355_msm_domain* d, void* d_out, const void* d_wires, const void* d_sigmas, const void* d_selectors,
                                                 const void* d_z, const void* d_pi, size_t m, size_t stride, size_t n, const void* ks,
                                                 const void* alpha, const void* beta, const void* gamma, const void* offset, unsigned flags,
                                                 void* stream);
RustError mi355_msm_domain_linear_combination(mi355_msm_domain* d, void* out, const void* const* cols, const size_t* lens, const void* coeffs,
                                              size_t m, unsigned flags);
RustError mi355_msm_domain_linear_combination_device(mi355_msm_domain* d, void* d_out, const void* const* d_cols, const size_t* lens,
                                                     const void* coeffs, size_t m, unsigned flags, void* stream);

/* ---- resident sparse matrices over Fr and y = M z (Groth16's witness map) ------------------------------------------------------------
 * The vectors a[i] = <A_i, z> and b[i] = <B_i, z> that open a Groth16 or Marlin prover: the rows of the R1CS matrices times the full
 * assignment (ark-groth16's evaluate_constraint loop over arkworks' Matrix<F>).  The matrices belong to the proving key, so like the
 * bases of an MSM they are uploaded once and kept; what changes per proof is z.
 *   create  CSR in HOST memory: row_ptr holds rows + 1 offsets (8-byte aligned), nnz = row_ptr[rows]; col_idx (4-byte aligned) and
 *           values hold nnz entries, a value being one 32-byte element: an arkworks Fr image or, with flag bit 0 (the only flag), a
 *           plain integer.  ANY 256-bit value is read as its residue.  Duplicate columns within a row are allowed and summed; zero
 *           coefficients, empty rows, rows == 0 and nnz == 0 are allowed.  rows, cols <= 2^30, nnz <= 2^31.  The field, the device, the
 *           stream of host-pointer calls and the work memory of the sum scan are those of the domain d, WHICH MUST OUTLIVE THE MATRIX;
 *           the vector lengths have nothing to do with the domain's size.  The structure is validated on the host before any device
 *           call: row_ptr[0] == 0, row_ptr non-decreasing, every col_idx < cols; a violation is -1 with a message that names the first
 *           offending row.  The call uploads once, converts the coefficients, synchronises and returns a handle that any number of
 *           apply calls reuse.
 *   apply   out[i] = sum_k values[k] * z[col_idx[k]] over the entries of row i: reads cols elements of z, writes rows canonical
 *           elements of out (an empty row gives 0; rows == 0 writes nothing).  Flag bit 0: z and out are plain integers -- the form of
 *           the call is independent of the form given at create.  Flag bit 1 (value 2): out and z are DEVICE pointers (4-byte
 *           aligned) and `stream` is the hipStream_t on which z becomes ready (NULL = the default stream): the work is enqueued there
 *           and the call returns when out is written, as the device-pointer calls of the domain do.  Without bit 1 both are host
 *           pointers, staged through buffers the matrix keeps, and a non-null stream is an error.  Any overlap of out and z is refused.
 *   query   "rows", "cols", "nnz"; "entries_per_lane" and "block_lanes", the constants E and L of the kernels (answered without a
 *           handle too); "work_bytes", everything the matrix holds on the device.
 * One apply with a flag bit, and no twin whose name ends in _device: every such name in this header stands in the table of
 * tests/stream_cases.py with the test that pins its stream order, and tests/test_stream_coverage.py keeps the two equal.  The
 * stream-ordering promise of flag bit 1 is the same one and is pinned by a late-producer test of its own in tests/test_gpu_sparse.py,
 * written with the helpers of stream_cases.
 * Scheme (csrc/sparse.hpp).  R1CS rows are badly skewed, so no kernel is per row: every lane handles E consecutive entries of the CSR
 * arrays, whatever rows they belong to.  create stores the coefficients as canonical Montgomery values of 32 bytes in a lane-interleaved
 * order, and per lane the row that is open at its first entry.  apply is five launches on one stream: z to class M, once per column;
 * the sum of every lane's E products; the exclusive prefix sum of the lane totals (the sum scan above); the lanes again, which write
 * every row that begins and ends inside a lane and leave the running sum where a row crosses a lane boundary; one lane per row for
 * those rows and the empty ones.  No block waits on another, nothing is atomic.  Sums in Fr are exact: results are canonical and never
 * depend on "poly_tile_log", on host versus device pointers or on the form of the call.  There is no CPU fallback.
 * Errors: -1 with a message, decided before any device call, in this order: unknown flag bits, sizes above their limits, null
 * pointers, alignment, a stream without flag bit 1, an output that overlaps z, the structure (create), and last the null handle
 * (create: the domain); the extent of an overlap is judged against the handle. */
typedef struct mi355_msm_sparse mi355_msm_sparse;
RustError mi355_msm_sparse_create(mi355_msm_sparse** out, mi355_msm_domain* d, size_t rows, size_t cols, const uint64_t* row_ptr,
                                  const uint32_t* col_idx, const void* values, unsigned flags);
RustError mi355_msm_sparse_apply(mi355_msm_sparse* m, void* out, const void* z, unsigned flags, void* stream);
RustError mi355_msm_sparse_query(mi355_msm_sparse* m, const char* key, uint64_t* value);
RustError mi355_msm_sparse_destroy(mi355_msm_sparse* m);

/* ---- dense multilinear extensions and sumcheck prover rounds over Fr (ark-poly's DenseMultilinearExtension, ark-linear-sumcheck) -------
 * The other half of ark-poly: a table of 2^num_vars evaluations over the boolean cube, and the prover's side of the sumcheck protocol
 * for g(x) = sum_j c_j prod_{k in S_j} f_k(x) (ListOfProductsOfPolynomials: Spartan, HyperPlonk, GKR, Lasso).  The calls live on the
 * domain handle, which lends its field, its stream for host-pointer calls, its host arithmetic and its work memory; the vector lengths
 * have nothing to do with the domain's size.  Index b of a table is the point (b_0, .., b_{nv-1}) with b_0 the lowest bit, and
 * variables are fixed from x_1 (the lowest bit) upward, as in ARK poly/src/evaluations/multivariate/multilinear/dense.rs.
 * Elements are 32 bytes: arkworks Fr images or, with flag bit 0, plain integers; ANY 256-bit input is read as its residue and every
 * output is canonical.  Flag bit 1 (value 2): the vectors are DEVICE pointers (4-byte aligned) and `stream` is the hipStream_t on which
 * the inputs become ready (NULL = the default stream): the work is enqueued there and the call returns when the outputs are written.
 * Without bit 1 they are host pointers, staged through buffers the handle keeps, and a non-null stream is an error.  Points,
 * challenges, term coefficients and round results are HOST elements in the form of the call, also with bit 1.
 *   mle_fix   fix_variables: out[b] = in[2b] + r (in[2b+1] - in[2b]) for r = point[0], then point[1] on the result, .., k times:
 *             0 <= k <= num_vars <= 30, in holds 2^num_vars elements, out 2^(num_vars - k).  k == num_vars is evaluate (one element);
 *             k == 0 writes the canonical copy.  out may not overlap in: a lane's pair is another block's output, so the fold cannot
 *             be done in place.  A tile through LDS fixes up to "poly_tile_log" variables in ONE pass, as a pass of the transform does
 *             several levels: evaluating a table reads it once, plus ceil(k / tile_log) - 1 much smaller passes that ping-pong through
 *             the handle's work memory.
 *   mle_eq    out[b] = prod_i (b_i ? point[i] : 1 - point[i]) for b < 2^k, k <= 30; k == 0 writes the one element 1.  Two half tables
 *             of 2^ceil(k/2) and 2^floor(k/2) entries are built in host arithmetic; the kernel is one product per output.
 *   sumcheck_round   one prover round.  `tables` is a HOST array of m pointers, 1 <= m <= 12, each a table of 2^num_vars elements,
 *             1 <= num_vars <= 30; `terms` a host array of 1 <= n_terms <= 8 records: a coefficient, a factor count 1 .. 5 and the
 *             factor indices, each below m (a repeated index is a power).  With d the largest factor count and r_prev == NULL:
 *               evals_out[t] = sum_{b < 2^(nv-1)} sum_j c_j prod_k (f_k[2b] + t (f_k[2b+1] - f_k[2b])),   t = 0 .. d
 *             -- d + 1 host elements, written when the call returns; there are no output vectors and `folded` is not read.  With
 *             r_prev the call first fixes x_1 = r_prev in every table, writes the m halved tables (2^(nv-1) elements each) to the m
 *             pointers of `folded`, none of which may overlap a table or another folded table, and returns the round evaluations of
 *             the FOLDED tables (nv - 1 variables, so num_vars >= 2), in the same pass over the inputs: round i of a prover is one
 *             read of every table and one write of half of it.  Lane sums, block sums, then the partial rows reduced by further
 *             launches; sums in Fr are exact, nothing is atomic, no block waits on another.
 *   query (mi355_msm_domain_query)   "mle_work_bytes"; "sumcheck_levels", the launches of the most recent round; "sumcheck_max_tables",
 *             "sumcheck_max_terms" and "sumcheck_max_factors", the limits above (answered without a handle too).
 * One call each with a flag bit, and no twin whose name ends in _device: this is the route mi355_msm_sparse_apply took, for the reason
 * given there; the stream-ordering promise of flag bit 1 is pinned by late-producer tests in tests/test_gpu_mle.py.
 * Results are canonical and never depend on "poly_tile_log", on host versus device pointers or on the form of the call.  There is no
 * CPU fallback.  Errors: -1 with a message, decided before any device call, in this order: unknown flag bits, sizes outside their
 * limits, null pointers, alignment, a stream without flag bit 1, overlap, the term list, and last the null handle. */
typedef struct mi355_msm_sumcheck_term {
  uint8_t coeff[32];
  uint32_t n_factors;
  uint32_t factors[5];
} mi355_msm_sumcheck_term;
RustError mi355_msm_domain_mle_fix(mi355_msm_domain* d, void* out, const void* in, unsigned num_vars, const void* point, unsigned k,
                                   unsigned flags, void* stream);
RustError mi355_msm_domain_mle_eq(mi355_msm_domain* d, void* out, const void* point, unsigned k, unsigned flags, void* stream);
RustError mi355_msm_domain_sumcheck_round(mi355_msm_domain* d, void* evals_out, const void* const* tables, size_t m, unsigned num_vars,
                                          const mi355_msm_sumcheck_term* terms, size_t n_terms, const void* r_prev, void* const* folded,
                                          unsigned flags, void* stream);

/* ---- Poseidon sponges and Merkle trees over Fr (snarkVM's PoseidonSponge, Poseidon::hash_many and its Poseidon Merkle tree) -----------
 * An algebraic hash on the device: batches of independent duplex sponges of one shape, and the Merkle tree built from them.  The
 * parameters belong to a system, so like a sparse matrix they are uploaded once and kept.  The state is [capacity | rate] with capacity
 * 1, t = rate + 1 elements; an absorbed element is ADDED to a rate cell; a round is ark, S-box x^alpha, mds; the rounds
 * full_rounds / 2 .. full_rounds / 2 + partial_rounds - 1 are partial, their S-box acts on element 0 alone
 * (console/algorithms/src/poseidon/helpers/sponge.rs).  Elements are 32 bytes: arkworks Fr images or, with flag bit 0, plain integers;
 * ANY 256-bit input is read as its residue and every output is canonical.
 *   create  1 <= rate <= 8; 3 <= alpha < 2^16, odd; full_rounds even, 2 .. 4096; partial_rounds 0 .. 4096.  ark holds
 *           (full_rounds + partial_rounds) * t HOST elements, round by round, mds t * t, row by row; flag bit 0 (the only flag): plain
 *           integers.  The caller always supplies the parameters: nothing about alpha = 17 or 8 + 31 rounds is in a kernel.  The field,
 *           the device, the stream of host-pointer calls and the host arithmetic are those of the domain d, WHICH MUST OUTLIVE THE
 *           HANDLE; nothing here has to do with the domain's size.  create derives the sparse form of the partial rounds (below) in host
 *           arithmetic and refuses, with a message that names the round, parameters for which it does not exist.
 *   hash    n <= 2^30 independent sponges: row i of `in` holds in_len <= 2^16 elements, row i of `out` receives n_out <= 2^16 squeezed
 *           elements.  `header`, if not NULL, is `rate` HOST elements in the form of the call (also with bit 1), absorbed before every
 *           row: with header = [domain, in_len, 0, ..] the call is Poseidon::hash_many, without it the raw sponge, absorb then squeeze.
 *           The duplex rules are the reference's: permute before absorbing into a full rate block, once before the first squeeze (an
 *           empty input still permutes once), and again when a squeeze passes `rate` outputs; n_out == 0 or n == 0 writes nothing.
 *   merkle  the Poseidon Merkle tree of console/collections/src/merkle_tree: leaf hash hash([0] || leaf), node hash
 *           hash([1, left, right]), empty hash hash([1, 0, 0]), hash(x) = hash_many(x, 1)[0] with the HOST element domain_sep as the
 *           domain.  1 <= n_leaves <= 2^30 leaves of leaf_len < 2^16 elements each; the rate must be at least 2.  tree_out receives the
 *           2P - 1 nodes, P = next_power_of_two(n_leaves), in the reference's order: the root of the built part at index 0, the
 *           children of node i at 2i + 1 and 2i + 2, the leaf hashes from P - 1 on, missing leaves holding the empty hash.  One launch
 *           of the hash kernel per level on one stream; levels are not fused.  The padding of root(depth) above the built part is a
 *           handful of node hashes and is left to the caller (hash with in_len 3).
 *   Flag bit 1 (value 2), hash and merkle: the vectors are DEVICE pointers (4-byte aligned) and `stream` is the hipStream_t on which
 *           the input becomes ready (NULL = the default stream): the work is enqueued there and the call returns when the output is
 *           written, as the device-pointer calls of the domain do.  Without bit 1 they are host pointers, staged through buffers the
 *           handle keeps, and a non-null stream is an error.  Any overlap of output and input is refused.
 *   set_option  "sparse": 1 (default), or 0 to run the partial rounds densely from the caller's ark and mds -- a test hook and the A/B of
 *           the measurement; the results are identical.
 *   query   "rate", "state" (t), "rounds", "sparse", "products_per_permutation" (Fr products of one permutation in the current form,
 *           the reductions below included), "lds_bytes" (per block), "work_bytes" (everything the handle holds on the device);
 *           "block_lanes", a constant of the kernel, is answered without a handle too.
 * One call each with a flag bit, and no twin whose name ends in _device: this is the route mi355_msm_sparse_apply took, for the reason
 * given there; the stream-ordering promise of flag bit 1 is pinned by late-producer tests in tests/test_gpu_poseidon.py.
 * Scheme (csrc/poseidon.hpp).  One lane per sponge; the state lives in LDS, lane-interleaved, and every loop is rolled, so one kernel
 * per field serves every rate; constants and matrices are indexed by the round counter and read on the scalar unit.  The linear layer N
 * of a partial round factors as N'' N' with N' = [[1, 0], [0, N^]] commuting with the partial S-box: N' moves backward into the round
 * constants and the previous layer, and a partial round costs the S-box and 2t - 1 products instead of t^2 (502 / 834 / 1690 products
 * per permutation at rate 2 / 4 / 8 with alpha 17 and 8 + 31 rounds, against 626 / 1330 / 3674).  Elements that skip a product grow
 * lazily; where a bound of csrc/fr.hpp would be passed (BLS12-381 only: 2^261 / r = 70.6) create schedules a product by 1, counted in
 * "products_per_permutation".  Results never depend on "sparse", on host versus device pointers or on the form of the call.  There is
 * no CPU fallback.
 * Errors: -1 with a message, decided before any device call, in this order: unknown flag bits, sizes outside their limits, null
 * pointers, alignment, a stream without flag bit 1, an output that overlaps the input, and last the null handle (create: the domain). */
typedef struct mi355_msm_poseidon mi355_msm_poseidon;
RustError mi355_msm_poseidon_create(mi355_msm_poseidon** out, mi355_msm_domain* d, unsigned rate, unsigned alpha, unsigned full_rounds,
                                    unsigned partial_rounds, const void* ark, const void* mds, unsigned flags);
RustError mi355_msm_poseidon_hash(mi355_msm_poseidon* p, void* out, const void* in, size_t n, size_t in_len, size_t n_out,
                                  const void* header, unsigned flags, void* stream);
RustError mi355_msm_poseidon_merkle(mi355_msm_poseidon* p, void* tree_out, const void* leaves, size_t n_leaves, size_t leaf_len,
                                    const void* domain_sep, unsigned flags, void* stream);
RustError mi355_msm_poseidon_set_option(mi355_msm_poseidon* p, const char* key, long value);
RustError mi355_msm_poseidon_query(mi355_msm_poseidon* p, const char* key, uint64_t* value);
RustError mi355_msm_poseidon_destroy(mi355_msm_poseidon* p);

/* ---- batch pairings and pairing products (arkworks / snarkVM Bls12::pairing and product_of_pairings, BLS12-377 and BLS12-381) ---------
 * What KZG openings, Groth16 proofs, BLS signatures and an SRS validation end in.  out[j] = prod_{i < group} e(P[j group + i], Q[j group + i]):
 * group = 1 gives batch pairings, group = n gives product_of_pairings.  The value is byte for byte the reference's
 * (curves/src/templates/bls12/bls12.rs): f_{|x|,Q}(P), conjugated for BLS12-381's negative x, raised to 3 (p^12 - 1) / r -- eprint 2016/130
 * Table 1 computes the cube of the reduced Tate power.  A pair whose P or Q is flagged infinity contributes 1; the flag byte is
 * authoritative.  P and Q must be of order r or flagged infinity: NOTHING is tested (mi355_msm_check_bases exists for that); for other
 * inputs the value is unspecified but the call is harmless, every loop has a fixed trip count and no access is indexed by data.  If the
 * Miller value is 0 -- impossible for points of order r; arkworks returns None -- the image is all zero and the check byte is 0.
 *   create  any of the four curve ids selects its family, as mi355_msm_domain_create does; device < 0: the current one.
 *   run     g1: n arkworks Affine<G1> images g1_stride bytes apart (at least 104), g2: n Affine<G2> images g2_stride apart (at least
 *           200), strides a multiple of 4, read exactly as mi355_msm_set_bases reads them.  n must be a multiple of group >= 1.  out
 *           receives n / group Gt images of 576 bytes: twelve 48-byte Fp elements in arkworks' order c0.c0.c0, c0.c0.c1, c0.c1.c0,
 *           c0.c1.c1, c0.c2.c0, c0.c2.c1, then the six of c1 (Fp12 = Fp6[w]/(w^2 - v), Fp6 = Fp2[v]/(v^3 - xi)); in-memory Montgomery
 *           images (R = 2^384, little-endian) like the coordinates of a point image, or with flag bit 0 canonical integers -- that is
 *           CanonicalSerialize of Fq12.  n == 0 writes nothing.
 *   check   the same inputs; ok receives one byte per group, 1 exactly when the product is one, and no Gt image leaves the device.
 *           Flag bit 0 has no meaning here and is refused.
 *   Flag bit 1 (value 2): every vector is a DEVICE pointer (4-byte aligned; ok needs none) and `stream` is the hipStream_t on which the
 *           inputs become ready (NULL = the default stream): the work is enqueued there and the call returns when the output is
 *           written.  Without bit 1 they are host pointers, staged through a buffer the handle keeps, and a non-null stream is an error.
 *   query   "workspace_bytes" (the two lane-interleaved workspaces), "work_bytes" (everything the handle holds on the device),
 *           "last_launches", "products_miller", "products_product_step", "products_final_exponentiation" (Fp products a lane
 *           executes), "program_ops", "device", "curve"; "block_lanes", "lane_bytes", "max_lanes" and "serial_group", constants of the kernels, are answered
 *           without a handle too.
 * One call each with a flag bit, and no twin whose name ends in _device: this is the route mi355_msm_sparse_apply and
 * mi355_msm_poseidon_hash took, for the reason given there; the stream-ordering promise of flag bit 1 is pinned by late-producer tests in
 * tests/test_gpu_pairing.py.  The handle belongs to one device; a sharded context plays no part.
 * Scheme (csrc/pairing.hpp).  Nothing above Fp2 is code: create writes the Miller loop, the product step and the final exponentiation
 * as lists of operations on Fp2 slots, and one rolled interpreter with a single Fp2 product runs them, one lane per pair (or run of
 * pairs) and per group; tower values live in a lane-interleaved workspace in device memory sized by the lanes in flight, not by n.
 * Groups of up to "serial_group" pairs are walked by one lane; larger ones are split over lanes and multiplied as a tree of fan-in 8
 * across lanes and blocks, without atomics and in an order fixed by the indices.  No prepared G2 tables.  There is no CPU fallback.
 * Errors: -1 with a message, decided before any device call, in this order: unknown flag bits; group == 0 or n not a multiple of
 * group; a stride too small or not a multiple of 4; null pointers (with n > 0); alignment; a stream without flag bit 1; an output that
 * overlaps an input; and last the null handle (create: a null out-pointer, then an unknown curve id). */
typedef struct mi355_msm_pairing mi355_msm_pairing;
RustError mi355_msm_pairing_create(mi355_msm_pairing** out, int curve, int device);
RustError mi355_msm_pairing_run(mi355_msm_pairing* h, void* out, const void* g1, size_t g1_stride, const void* g2, size_t g2_stride,
                                size_t n, size_t group, unsigned flags, void* stream);
RustError mi355_msm_pairing_check(mi355_msm_pairing* h, uint8_t* ok, const void* g1, size_t g1_stride, const void* g2, size_t g2_stride,
                                  size_t n, size_t group, unsigned flags, void* stream);
RustError mi355_msm_pairing_query(mi355_msm_pairing* h, const char* key, uint64_t* value);
RustError mi355_msm_pairing_destroy(mi355_msm_pairing* h);

/* ---- batch hash-to-curve (RFC 9380; arkworks MapToCurveBasedHasher over WBMap with DefaultFieldHasher<Sha256, 128>; BLS12-381 G1 and G2) ----
 * What a BLS verification starts with: H(m).  The suites are BLS12381G1_XMD:SHA-256_SSWU_RO_ and BLS12381G2_XMD:SHA-256_SSWU_RO_ (hash) and
 * their _NU_ forms (encode), byte for byte RFC 9380's vectors as the arkworks tests read them.  A handle is made for one curve
 * (MI355_BLS12_381_G1 or MI355_BLS12_381_G2) and one domain separation tag; both BLS12-377 curves are refused at create: no standard
 * suite exists for them.
 *   create  dst: 1 .. 255 bytes are used as they are; a longer tag is replaced by SHA-256("H2C-OVERSIZE-DST-" || dst) (RFC 9380 5.3.3).
 *           device < 0: the current one.
 *   field   hash_to_field: n messages as one byte buffer `data` of data_bytes bytes and n + 1 64-bit offsets (message i is
 *           data[offsets[i] .. offsets[i + 1])); count 1 or 2; out receives count * m base-field images per message (m = 1 for G1, 2 for
 *           G2), 48 bytes each, in the form the coordinates of an Affine image have (Montgomery, R = 2^384, little-endian), c0 before c1.
 *           Host pointers: the offsets must be non-decreasing and end inside the buffer, which is checked before anything is
 *           launched.  Device pointers: the offsets are not read on the host; the kernel clamps every message to the buffer, so a bad
 *           offset cannot read outside it.  A message is shorter than 2^28 bytes.
 *   map     n field images (48 m bytes each, packed) -> n points: simplified SWU on the isogenous curve, then the isogeny (WBMap::
 *           map_to_curve; NO cofactor clearing: the points are on the curve, not in the subgroup).  With flag bit 2 (pairs) n must be
 *           even and out receives n / 2 points clear_cofactor(map(u[2j]) + map(u[2j + 1])).
 *   hash    messages as for field -> n points: hash_to_curve (two u per message, add, clear the cofactor); with flag bit 0
 *           encode_to_curve (one u, clear).
 *   Output: arkworks Affine images out_stride bytes apart (a multiple of 4, at least the image: 104 / 200 bytes), infinity as zeros
 *           with the flag byte set; flag bit 3: normalised Projective images (144 / 288 bytes), as mi355_msm_mul_points writes them.
 *   Flag bit 1 (value 2): every vector is a DEVICE pointer (4-byte aligned, offsets 8-byte) and `stream` is the hipStream_t on which
 *           the inputs become ready (NULL = the default stream): the work is enqueued there and the call returns when the output is
 *           written.  Without bit 1 they are host pointers, staged through a buffer the handle keeps, and a non-null stream is an error.
 *   query   "work_bytes" (everything the handle holds on the device), "lanes_in_flight" (the widest launch of the last call),
 *           "last_launches", "device", "curve", "dst_bytes", "dst_oversize"; "block_lanes" and "max_lanes", constants of the
 *           kernels, are answered without a handle too.
 * One call each with a flag bit, and no twin whose name ends in _device, as the pairing handle has it; the stream-ordering promise of
 * flag bit 1 is pinned by a late-producer test in tests/test_gpu_h2c.py.  The handle belongs to one device.
 * Scheme (csrc/h2c.hpp).  expand_message_xmd and the reduction run one lane per message with SHA-256 in registers: meant for short
 * messages (32 .. 200 bytes); a lane per message is a poor shape for kilobyte messages, which work but serialise a wave on its
 * longest.  The map runs one lane per u, division-free, sqrt_ratio as one exponentiation, the isogeny by Horner on the projective x;
 * G1 clears the cofactor by h_eff = 1 - z, G2 by psi (Budroni-Pintore), which equals h_eff Q on every point of the curve.  Work
 * buffers are sized by the lanes in flight ("max_lanes"), never by n -- but for the staging buffer of a host-pointer call, which holds
 * that call's whole input, offsets and packed output.  Every constant is derived from the suite parameters by
 * tools/gen_h2c_consts.py.  There is no CPU fallback.
 * Errors: -1 with a message, decided before any device call, in this order: unknown flag bits; count / an odd n with pairs; the
 * stride; null pointers (with n > 0); alignment; a stream without flag bit 1; bad offsets (host pointers); and last the null handle
 * (then the stride against the handle's image, and overlap).  create: a null out-pointer, an unknown curve id, an empty tag, a
 * BLS12-377 curve, then the device. */
typedef struct mi355_msm_h2c mi355_msm_h2c;
RustError mi355_msm_h2c_create(mi355_msm_h2c** out, int curve, const void* dst, size_t dst_len, int device);
RustError mi355_msm_h2c_field(mi355_msm_h2c* h, void* out, const void* data, size_t data_bytes, const uint64_t* offsets, size_t n,
                              unsigned count, unsigned flags, void* stream);
RustError mi355_msm_h2c_map(mi355_msm_h2c* h, void* out, size_t out_stride, const void* u, size_t n, unsigned flags, void* stream);
RustError mi355_msm_h2c_hash(mi355_msm_h2c* h, void* out, size_t out_stride, const void* data, size_t data_bytes, const uint64_t* offsets,
                             size_t n, unsigned flags, void* stream);
RustError mi355_msm_h2c_query(mi355_msm_h2c* h, const char* key, uint64_t* value);
RustError mi355_msm_h2c_destroy(mi355_msm_h2c* h);

/* ---- transforms of vectors of curve points over a domain (ARK poly/src/domain/mod.rs:99-170 on DomainCoeff = G1Projective / G2Projective) ----
 * domain.fft / ifft / coset_fft / coset_ifft on GROUP elements: what turns a monomial SRS [tau^j] G into the Lagrange SRS
 * [L_i(tau)] G (kind 1), and the transform behind FK20, cq and Caulk tables.  With in[j] a point and the products scalar multiples:
 *   kind     0 forward    out[i] = sum_{j<n} omega^(i j) * in[j]
 *            1 inverse    out[j] = n^-1 * sum_{i<n} omega^(-i j) * in[i]
 *            2 coset forward   out[i] = sum_j (g omega^i)^j * in[j]
 *            3 coset inverse   out[j] = g^-j * n^-1 * sum_i omega^(-i j) * in[i]
 * Every multiplier is the canonical integer below r of the field element, as arkworks' MulAssign<Fr> uses.  Natural order in and out.
 *   ctx      a single-device context of the curve whose points these are; domain: a handle of the same curve FAMILY on the same
 *            device (n = its size, omega, the tables).  The context's base set plays no part.
 *   in       in_len <= n arkworks Affine images, `stride` bytes apart (a multiple of 4, at least two coordinates and the flag byte),
 *            read as mi355_msm_mul_points reads them: the flag byte is authoritative, infinities are allowed anywhere, and NOTHING is
 *            tested.  Points from in_len on are the point at infinity and their bytes are never read; in may be NULL when in_len is 0
 *            (the call then writes n infinities).  The points must lie in the order-r subgroup for the result to be the sums above;
 *            for other records the result is unspecified, but the call finishes: every memory access is a function of the lane
 *            index, n and the twiddle's digits alone.
 *   offset   g: a HOST pointer (also in the _device call) to one 32-byte arkworks Fr image; NULL = GENERATOR.  Kinds 2 and 3 only;
 *            zero is refused.
 *   out      n images, out_stride bytes apart (a multiple of 4, at least the image size; bytes between two images are not written).
 *            Default: Affine images -- x, y canonical, every flag and pad byte written, infinity all zeros with flag 1.  Flag bit 1:
 *            normalised Projective images, as mi355_msm_mul_points writes them.  No other flag bit exists.
 *            out == in with out_stride == stride is allowed; any other overlap of the bytes read with the bytes written is refused.
 * n = 1 copies (normalises) the point.
 * The transform is k = log2 n stages of n / 2 butterflies T = w * B, A' = A + T, B' = A - T, decimation in time in Stockham's
 * self-sorting layout (csrc/group_fft.hpp): every stage reads through an index map and writes two contiguous runs, so no launch
 * permutes.  One lane per butterfly: the twiddle LO[e mod 2^14] * HI[e >> 14] from the domain's tables becomes a canonical integer in
 * registers, its signed digits walk B's table (built and normalised per stage, as mul_points builds one), and the two mixed additions
 * of the affine A onto T and -T follow in the same kernel.  Stage 0 has twiddle 1 everywhere and multiplies nothing: a forward
 * transform costs (n / 2)(k - 1) multiplications; a coset forward transform one more per point (by g^j, before the stages), an inverse
 * one more per point (by n^-1 or g^-j n^-1 as one factor, after them).  Between two stages the vector is normalised back to Affine
 * images by the batched normalisation.
 * Work memory, kept by the context (query "fft_points_work_bytes"): two vectors of n packed Affine images, the chunk buffers of one
 * stage -- sized like mul_points': the largest power of two within its 2 GiB bound, 2^19 butterflies for G1 and 2^18 for G2, which
 * take 1.6 GiB at the default window -- and, for host-pointer calls, the staged input and output.  Options: "fft_points_chunk", butterflies per chunk (0 restores the default; a test hook);
 * "mul_window" applies as it stands.  Results never depend on either, nor on host versus device pointers.
 * Queries: "fft_points_chunk", "fft_points_work_bytes", "last_fft_points_us" (host clock around the most recent call),
 * "last_fft_points_device_us" (the same call between events on the stream it ran on).
 * mi355_msm_fft_points takes HOST pointers; mi355_msm_fft_points_device DEVICE pointers (4-byte aligned) and the hipStream_t on which
 * the input becomes ready (NULL = the default stream): the work is enqueued there and the call returns when the output is written.
 * Errors: -1 with a message for an unknown kind, unknown flag bits, an offset on kinds 0 and 1, a zero offset, null handles, a sharded
 * context, a domain of the other curve family or on another device, in_len > n, bad strides, null pointers, a partial overlap, a size
 * whose two work vectors exceed 64 GiB -- decided before any device call; hipErrorNoDevice without a GPU (no handle can be created).
 * Measured on one MI355X (tools/gfft_bench.py, profiles/gfft.txt: device-resident subgroup points, host clock, beside pairwise
 * mul_points on the same points; the count gives (k - 1) / 2 multiplications per point forward, one more for the inverse kinds):
 * BLS12-381 G1 at 2^20 points forward 403 ms, inverse 452 ms, coset inverse 453 ms -- 9.0, 10.1 and 10.1 times mul_points against a
 * count of 9.5 and 10.5; BLS12-377 G1 387 / 434 / 435 ms.  At 2^16 a stage no longer fills the device and the ratio tends to k - 1:
 * BLS12-381 G1 89 / 96 / 96 ms (14.3 / 15.4 / 15.4 times), G2 243 / 262 / 262 ms (14.2 / 15.3 / 15.4 times); at 2^12 63 / 69 / 69 ms and
 * 168 / 185 / 186 ms (11 and 12 times).  Not measured: sizes above 2^20, G2 above 2^16, the coset forward transform, host-pointer calls,
 * Projective output, and any kernel-level profile. */
RustError mi355_msm_fft_points(mi355_msm_ctx* ctx, mi355_msm_domain* domain, void* out, size_t out_stride, const void* in, size_t in_len,
                               size_t stride, unsigned kind, unsigned flags, const void* offset);
RustError mi355_msm_fft_points_device(mi355_msm_ctx* ctx, mi355_msm_domain* domain, void* d_out, size_t out_stride, const void* d_in, size_t in_len,
                                      size_t stride, unsigned kind, unsigned flags, const void* offset, void* stream);

/* ---- lookup-argument columns over Fr: resident lookup tables (logUp multiplicities, plookup's sorted vector) and the logUp running sum ----
 * The step every Plonk-style prover has between "wires committed" and "grand product / running sum": halo2, UltraPlonk / Jellyfish,
 * Plonkup and logUp in its univariate and its sumcheck form all join a witness column against a table.  The contract is stated on
 * integers.  Elements are 32 bytes: arkworks Fr images or, with flag bit 0, plain integers; ANY 256-bit pattern is read as its
 * residue, and every Fr output is canonical.  Flag bit 1 (value 2): the vectors are DEVICE pointers (4-byte aligned) and `stream` is
 * the hipStream_t on which the inputs become ready (NULL = the default stream); the work is enqueued there and the call returns when
 * its outputs are written.  Without bit 1 they are host pointers, staged through buffers the handle keeps, and a non-null stream is an
 * error.  `stats`, `beta` and `total32` are HOST memory in both cases.
 *   create  the table t[0 .. n_t), 1 <= n_t <= 2^28, on the field, the device, the events and the host-pointer stream of the domain d,
 *           WHICH MUST OUTLIVE THE TABLE (its size plays no part).  Equality is equality MODULO r: v, v + r, v + 2r, .. match each
 *           other wherever they fit 256 bits.  The matching key is the canonical residue of the 256-bit pattern in the form of the
 *           call; Montgomery images are in bijection with residues, so matching needs a reduction and no field product.  The table is
 *           fixed for the life of the handle IN THE FORM IT WAS CREATED WITH: a later call whose flag bit 0 differs is refused.
 *           Duplicates are allowed: first(i) is the smallest j with t[j] == t[i], and every match is credited to the first occurrence.
 *   count   for n_f <= 2^30 values: index_out[j] (n_f u32; may be NULL) = first(i) for the t[i] == values[j], or 0xFFFFFFFF when there
 *           is none; mult_out[i] (n_t elements in the form of the call; may be NULL) = the number of j with index_out[j] == i, so 0 at
 *           later duplicates; stats[0] = the number of values without a match, stats[1] = the smallest such j, or n_f when there is
 *           none.  A MISSING VALUE IS NOT AN ERROR (as a zero denominator is none in the permutation product).  n_f == 0 writes n_t
 *           zeros and stats (0, 0).
 *   sorted  s_out receives the n_t + n_f elements of plookup's s = (f, t) sorted by t: for i = 0 .. n_t - 1 in order t[i], followed
 *           by mult[i] further copies of t[i], all canonical in the form of the call.  If stats[0] != 0 NOTHING is written to s_out
 *           and the call still returns 0.  Jellyfish's h1 = s[:n], h2 = s[n-1:] and the alternating halves of Plonkup are slices of
 *           s_out for the caller to take.
 *   query   "n", "slots", "distinct" (keys), "max_probe" (the longest probe walk of the build), "table_bytes" (keys and slots),
 *           "lookup_work_bytes" (counters, offsets, scan levels, staged vectors).
 *   mi355_msm_domain_logup_sum   n <= 2^30 rows, any n; values holds 1 <= m <= 8 columns of n elements, stride >= n elements apart;
 *           beta is one HOST element.  term[j] = sum_c 1 / (beta + values_c[j]) - mult[j] / (beta + table[j]); out[0] = 0,
 *           out[j + 1] = out[j] + term[j] (n elements, exclusive); total32 (may be NULL) = out[n-1] + term[n-1], which is 0 exactly
 *           when the multiset relation holds; helpers (may be NULL) receives (m + 1) n elements: the m columns 1 / (beta +
 *           values_c[j]), then mult[j] / (beta + table[j]) -- what sumcheck-based logUp commits to instead of the running sum.
 *           A ZERO DENOMINATOR IS NOT AN ERROR: the batch inversion leaves it zero and that term contributes 0 (as the permutation
 *           product documents).  Neither output may overlap an input or the other output.  n == 0 writes total32 = 0 only.
 * No name here ends in _device: every such name in this header stands in the table of tests/stream_cases.py, and
 * tests/test_stream_coverage.py keeps the two equal.  The stream-ordering promise of flag bit 1 is the same one and is pinned by
 * late-producer tests of its own in tests/test_gpu_lookup.py, one each for create, count, sorted and logup_sum.
 * Scheme (csrc/lookup.hpp).  create: one launch reduces the table into the handle's canonical copy; one launch inserts, a lane per
 * entry, open addressing with linear probing into `slots` = the power of two >= 2 n_t of u32 indices.  The hash mixes all eight words
 * of the key (murmur3).  An empty slot is claimed with a compare-and-swap; a slot whose entry is equal is lowered with an atomic min,
 * which makes first(i) independent of the arrival order; slots are read through agent-scope atomic loads.  count: a separate launch,
 * a lane per value, walks with plain loads, writes index_out and adds to a u32 counter AFTER the lanes of a wave that found the same
 * entry have combined into one add (a padded column puts most values on one counter; a heavy entry and the misses are carried over
 * the values a block takes and added once per block, since adds to one address are serialised); the missing count and the first missing
 * index are two 64-bit atomics per block that has misses; one lane per entry writes the counter as an element (at most one product).  sorted:
 * the same probe, an exclusive u32 scan of 1 + count (tiles of 1024, levels as launches), and one lane per OUTPUT element that finds
 * its entry by bisection -- balanced whatever the distribution.  No lane waits on another lane's progress, a walk is bounded by
 * `slots`, nothing is polled; a walk that wraps (impossible at load <= 1/2) is error -2.  Sums and minima of integers do not depend
 * on their order: every output byte is a function of the inputs alone.  logup_sum: one launch writes the (m + 1) n denominators, the
 * three launches of the batch inversion run over them in place, one launch forms the last helper column and the row's term, and the
 * sum scan runs over the terms.  Work memory is the domain's (query "logup_work_bytes"; the other queries keep their values).
 * Results never depend on host versus device pointers.  There is no CPU fallback.
 * Errors: -1 with a message, decided before any device call, in this order: unknown flag bits, sizes outside their limits, null
 * pointers, alignment, a stream without flag bit 1, an overlap, and last the null handle (create and logup_sum: the domain), after
 * which the extent of an overlap and the form of the table are judged against the handle.  hipErrorNoDevice without a GPU. */
typedef struct mi355_msm_lookup mi355_msm_lookup;
RustError mi355_msm_lookup_create(mi355_msm_lookup** out, mi355_msm_domain* d, const void* table, size_t n_t, unsigned flags, void* stream);
RustError mi355_msm_lookup_count(mi355_msm_lookup* h, void* mult_out, uint32_t* index_out, uint64_t* stats, const void* values, size_t n_f,
                                 unsigned flags, void* stream);
RustError mi355_msm_lookup_sorted(mi355_msm_lookup* h, void* s_out, uint64_t* stats, const void* values, size_t n_f, unsigned flags, void* stream);
RustError mi355_msm_lookup_query(mi355_msm_lookup* h, const char* key, uint64_t* value);
RustError mi355_msm_lookup_destroy(mi355_msm_lookup* h);
RustError mi355_msm_domain_logup_sum(mi355_msm_domain* d, void* out, void* total32, void* helpers, const void* table, const void* mult,
                                     const void* values, size_t m, size_t stride, size_t n, const void* beta, unsigned flags, void* stream);

/* ---- custom-gate expressions over Fr columns with rotations: a DAG compiled once, evaluated for every row in one launch ----
 * What a Plonkish (halo2-style) prover computes in its quotient round and halo2 calls evaluate_h: a circuit-specific polynomial
 * expression in dozens of columns read at several rotations.  mi355_msm_domain_plonk_quotient has Jellyfish's gate wired in; this
 * handle evaluates any gate.  The contract is stated on integers: out[i] = the DAG evaluated modulo r at row i.
 *   create  on the field and the device of the domain d, WHICH MUST OUTLIVE THE PROGRAM (its size plays no part).  `nodes` holds
 *           n_nodes triples (op, a, b) of uint32_t in topological order, the last one the result:
 *             0 COL    column a at the rotation b (a signed 32-bit value, within +-2^15)
 *             1 CONST  element a of `consts` (n_consts 32-byte HOST elements; flag bit 0 at create: plain integers)
 *             2 CHAL   element a of the challenges given at every run
 *             3 ADD, 4 SUB, 5 MUL of the earlier nodes a and b;  6 NEG, 7 SQR of the earlier node a
 *           At most 65 535 nodes, 4 096 constants, 64 challenges, 64 columns.  Nodes the result does not depend on cost nothing.
 *           create FAILS (-1, the message names S and the limit) when the program needs more than 32 slots at once: split the sum
 *           over an output column (overlap rule below).
 *   run     out[i], i < len <= 2^30 (any len, not only a power of two; len == 0 succeeds and writes nothing).  `cols` is a HOST array
 *           of ncols pointers, lens[j] the length of column j, which must divide len: COL(j, rot) is read at row
 *           ((i + rot * rot_step) mod len) mod lens[j].  A periodic column (the `ratio` inverses of Z_H on a coset) costs its period,
 *           a column of length 1 is a scalar.  rot_step is M / n on a quotient domain, 1 on the constraint domain.  `challenges`:
 *           nchal HOST elements.  Flag bit 0: plain integers instead of arkworks images -- columns, challenges and output alike; ANY
 *           256-bit input is read as its residue and every output is canonical.  Flag bit 1 (value 2): the pointers in `cols` and
 *           `out` are DEVICE pointers (4-byte aligned), `stream` is the hipStream_t on which the inputs become ready, the work is
 *           enqueued there and the call returns when the output is written; without it they are host pointers, staged through a buffer
 *           the program keeps, and a non-null stream is an error.  OVERLAP: `out` may BE one of the full-length columns if the program
 *           reads that column at rotation 0 only; any other overlap of out with a column is refused.
 *   query   "nodes", "instructions", "slots" (S), "products" (field products per row, the conversions of the column operands and of
 *           the result included), "reduces" (reductions the compiler inserted), "columns", "lds_bytes" (per block of 64 rows),
 *           "last_us", "last_device_us".
 * No name here ends in _device (the convention of mi355_msm_lookup_count); tests/test_gpu_expr.py pins the stream-ordering promise of
 * flag bit 1 with a late producer.
 * Scheme (csrc/expr.hpp).  create orders the evaluation by a post-order walk that takes the operand with the larger Sethi-Ullman label
 * first, then hands out slots by a linear scan: leaves are never kept (a column operand is loaded at its use and pays its one
 * conversion there, constants and challenges are read through wave-uniform pointers), a node whose only use is the next instruction
 * stays in registers, every other interior node keeps a slot until its last use.  A slot is 8 words per lane: every stored value is a
 * 256-bit integer below 2^256, which is tighter than what a product asks of its operands, so the compiler carries an upper bound in
 * units of r for every node and inserts a reduction (a conditional subtraction of r, or a product by one when the bound is above 3)
 * where an ADD, SUB or NEG would otherwise pass 2^256 / r = 13.7 (BLS12-377) or 2.2 (BLS12-381).  run: ONE launch, one lane per row, blocks
 * of one wave; the slots live in dynamic LDS, lane-interleaved (no lane reads another's, no barrier); the instruction loop is rolled
 * and its control is wave-uniform; only the column reads are indexed by the lane.
 * Work memory is the program's own: the instructions and constants, the column references and challenges of the most recent run, the
 * staged vectors of a host-pointer run.  Results never depend on host versus device pointers.  There is no CPU fallback.
 * Errors: -1 with a message, decided before any device call: unknown flag bits, len above 2^30, more than 64 columns or challenges,
 * null pointers, a lens[j] of 0 or one that does not divide len, alignment, a stream without flag bit 1, an overlap in part, and last
 * the null handle (create: the limits of the DAG, then the domain), after which ncols and nchal are judged against what the program was
 * created with, and an `out` that is a column against its rotations.  hipErrorNoDevice without a GPU. */
typedef struct mi355_msm_expr mi355_msm_expr;
RustError mi355_msm_expr_create(mi355_msm_expr** out, mi355_msm_domain* d, const uint32_t* nodes, size_t n_nodes, const void* consts, size_t n_consts,
                                size_t n_chal, size_t n_cols, unsigned flags);
RustError mi355_msm_expr_run(mi355_msm_expr* e, void* out, const void* const* cols, const size_t* lens, size_t ncols, size_t len, size_t rot_step,
                             const void* challenges, size_t nchal, unsigned flags, void* stream);
RustError mi355_msm_expr_query(mi355_msm_expr* e, const char* key, uint64_t* value);
RustError mi355_msm_expr_destroy(mi355_msm_expr* e);

/* ---- segmented MSM: many small MSMs in one call ------------------------------------------------------------------------------------
 * S independent sums in one launch chain -- the h-vector of FK20 / PeerDAS cell proofs (128 MSMs of 64 points per blob), the short
 * columns of a circuit over one SRS, IPA and Verkle rounds, committee key aggregation.  mi355_msm_run is built for one sum of 2^20 to
 * 2^26 pairs; this call for sums of 1 to a few thousand terms (longer segments are legal and slow: they are mi355_msm_run's job).
 *   general  (flag bit 2 clear) `offsets` is a HOST array of nsegments + 1 values, offsets[0] = 0, non-decreasing,
 *            offsets[nsegments] = npoints = nscalars;  out[s] = sum over i in [offsets[s], offsets[s+1]) of scalars[i] * points[i].
 *            An empty segment gives the point at infinity.  `offsets` is host memory also with device pointers: it is the shape of
 *            the call, and the launch plan is built from it.
 *   shared   (flag bit 2, value 4) `offsets` must be NULL and nscalars = nsegments * npoints;
 *            out[s] = sum over i < npoints of scalars[s * npoints + i] * points[i]: one set of bases serves every member.
 *   points   Affine images `stride` bytes apart, read exactly as mi355_msm_mul_points reads them: the flag byte is authoritative,
 *            infinities are allowed anywhere, no curve test and no subgroup test.  A record on no curve gives an unspecified result;
 *            the call still finishes without a fault.
 *   scalars  32-byte little-endian integers; all 256 bits count, nothing is reduced modulo r.  Flag bit 0 (value 1): arkworks Fr
 *            images, converted first.
 *   out      one image per segment, out_stride bytes apart (a multiple of 4, at least the image size).  Default: Affine images with
 *            every flag and pad byte written, as mi355_msm_mul_points writes them -- ready for set_bases, fft_points,
 *            compress_points and the pairing calls.  Flag bit 3 (value 8): normalised Projective images, the bytes mi355_msm_run
 *            returns.  `out` must not overlap an input.
 *   pointers flag bit 1 (value 2): points, scalars and out are DEVICE pointers (4-byte aligned) and `stream` is the hipStream_t on
 *            which they become ready (NULL = the default stream); the work is enqueued there and the call returns when the output is
 *            written.  Without bit 1 they are host pointers and a non-null stream is an error; the points, the scalars and the
 *            packed output are staged WHOLE in device buffers the context keeps (npoints * stride + 32 * nscalars bytes: unlike
 *            mul_points the call is not chunked over its inputs, only over its segments' work memory), so a call near the 2^32
 *            limit belongs to the device-pointer form.
 * The bytes of out[s] depend on the pairs of segment s alone: never on the window size, the tile length, the chunking, the pointer
 * kind, the form, or what the neighbouring segments hold.  nsegments = 0 succeeds and writes nothing.
 * Options (mi355_msm_set_option; test hooks, readable through mi355_msm_query): "seg_window" 1..9 (0 = by the segment's length:
 * 4 up to 256 pairs, 5 up to 768, 6 up to 2560, 7 up to 8192, 8 up to 16384, 9 beyond), "seg_tile" (an UPPER BOUND on the points per sorting tile, a
 * power of two from 64 to 4096; 0 = 1024: a class of segments runs with the largest power of two that is within it, within 20 KiB
 * of LDS a block and not longer than its longest segment needs -- at most 256 at window size 4, 512 at 5), "seg_chunk" (segments per chunk; 0 = as many as 2 GiB of work memory hold).  Queries also:
 * "seg_work_bytes", "last_segments_us", "last_segments_device_us".
 * Errors: -1 with a message that names the argument -- null pointers where a length is non-zero, a stride too small or not a multiple
 * of 4, offsets that do not start at 0, that decrease or that do not end at npoints (the message names the first offending index),
 * the shared form with offsets or a wrong nscalars, npoints >= 2^32, unknown flag bits, out overlapping an input, a sharded context,
 * a stream with host pointers -- decided before any device call; hipErrorNoDevice without a GPU. */
RustError mi355_msm_segments(mi355_msm_ctx* ctx, const void* points, size_t npoints, size_t stride, const void* scalars, size_t nscalars,
                             const uint64_t* offsets, size_t nsegments, unsigned flags, void* out, size_t out_stride, void* stream);

/* Sum `count` projective images (any Z) into one normalised image: the multi-GPU combine step
 * ("final 8-point curve add").  Pure host arithmetic on <= a few dozen points; no device needed. */
RustError mi355_msm_fold(int curve, void* out_projective, const void* projective, size_t count);

/* Synthetic bases in the shape of the reference harness generator (P1A yrrid/src/util.rs:15-28): `distinct`
 * subgroup points (h0 + j*h1)*G derived from `seed`, written as arkworks Affine images `stride` bytes apart into
 * HOST memory and replicated by doubling the vector up to `npoints`.  Host arithmetic; no device needed. */
RustError mi355_msm_generate_points(int curve, uint64_t seed, size_t distinct, size_t npoints, void* out_affine,
                                    size_t stride);

/* The execution plan the engine would use for an MSM of `npoints` pairs (pure host arithmetic, no device): out[0..9] =
 * window bits, digit windows, windows owning buckets (1 with precompute), sorted entries, entries per lane, lanes,
 * fragment-merge launches, bucket-reduce launches, sort key bits, bytes of per-run device work buffers.
 * `options` may be NULL or {window_bits, lane_entries, seg_entries} (0 = automatic).  `precompute`: 0 = no tables, 1 = a table
 * level per window, k > 1 = the context option "table_levels" = k -- the plan then equals what a context with those options
 * reports through mi355_msm_query "table_window_bits" / "table_levels".
 * NOTE: this argument is a LEVEL COUNT, not the context option "precompute" (where 2 means "auto"): passing that option's value here
 * plans two table levels.  To plan what an auto context runs, query its "table_levels" after set_bases and pass that. */
RustError mi355_msm_plan(int curve, size_t npoints, int precompute, const long* options, uint64_t* out);

/* The slice [*lo, *hi) of range(npoints) that shard `shard` of `nshards` owns in a sharded context (and in dist.py's
 * one-process-per-GPU path): ceil(npoints / nshards) consecutive pairs per shard, the last ones possibly shorter or empty.
 * Pure host arithmetic. */
RustError mi355_msm_shard_bounds(size_t npoints, int nshards, int shard, size_t* lo, size_t* hi);

/* Library/ABI version and the gfx target the kernels were built for ("gfx950"). */
const char* mi355_msm_version(void);

#ifdef __cplusplus
}
#endif
#endif /* MI355_MSM_H */
