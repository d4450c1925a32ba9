/* libzkmi355x -- C-ABI of the MI355X-native Groth16 / Pinocchio prove path for zukelang.
 *
 * This is the drop-in boundary: plain pointers and sizes, no C++ or torch types.  Every entry
 * point names the reference interface it replaces (paths relative to the zukelang tree).  The
 * OCaml ctypes stubs a maintainer would add are shown in INTEGRATION.md.
 *
 * Byte formats (what the OCaml side already holds):
 *   Fr      32 B little-endian canonical integer < r            (Bls12_381.Fr.to_bytes)
 *   G1      96 B uncompressed ZCash big-endian x || y           (G1.to_bytes, curve.ml:161)
 *   G2     192 B uncompressed x1 || x0 || y1 || y0              (G2.to_bytes)
 *   infinity: first byte 0x40, rest zero -- the ONE encoding of the identity: every decoder (uncompressed and compressed, host and device) refuses a
 *   string whose infinity bit is set next to the sign bit, another bit of the first byte or a non-zero byte anywhere (ZK_ERR_ARG).
 *   Compressed outputs (48 B / 96 B) carry the 0x80 / 0x40 / 0x20 flag bits of
 *   to_compressed_bytes (curve.ml:199,208) -- the JSON form of proofs (groth16.ml:110-114).
 *
 * Ownership: all buffers are caller-owned; the library copies host->device and retains no host
 * pointer after return.  Long-lived device state sits behind uint64_t handles with explicit free.
 * Threading: calls are synchronous and blocking (the reference is single-threaded OCaml) and are made from ONE host thread.  One process drives
 * one GPU by default; with a device list of several entries (zk_set_devices) the SAME single-threaded calls drive all of them: a key uploaded
 * through zk_groth16_pk_upload is then sharded over the list behind one handle (see "multi-device keys" below).
 * Errors: 0 = ok, negative = the codes below (the reference raises exceptions; the shim maps
 * ZK_ERR_APPLY_POWERS -> Invalid_argument "apply_powers", ZK_ERR_REMAINDER / ZK_ERR_DOMAIN ->
 * Assert_failure, the rest -> Failure (zk_strerror)).
 */
#ifndef ZKMI355X_H
#define ZKMI355X_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

#define ZK_OK 0
#define ZK_ERR_ARG (-1)            /* bad length / null pointer / unsupported size */
#define ZK_ERR_NOT_ON_CURVE (-2)   /* a base point fails y^2 = x^3 + b */
#define ZK_ERR_SCALAR_RANGE (-3)   /* an Fr input is >= r */
#define ZK_ERR_REMAINDER (-4)      /* p mod Z != 0: `assert (Polynomial.is_zero rem)`, src/lib/zk/QAP.ml:134 */
#define ZK_ERR_HIP (-5)            /* HIP runtime error (no GPU, OOM, launch failure) */
#define ZK_ERR_APPLY_POWERS (-6)   /* fewer points than coefficients: invalid_arg "apply_powers", src/lib/zk/curve.ml:116 */
#define ZK_ERR_HANDLE (-7)         /* unknown or freed handle */
#define ZK_ERR_DOMAIN (-8)         /* key sets differ: `assert false` in G.dot, src/lib/zk/curve.ml:96-100 */

const char* zk_strerror(int code);
const char* zk_last_error(void);       /* detail of the most recent failure in this process */
int zk_device_count(void);             /* number of visible HIP devices (0 without a GPU) */
int zk_init(int device);               /* bind this process to one GPU (a device list of one entry); idempotent */
int zk_shutdown(void);
/* ---- multi-device keys: N GPUs of one node behind the handle `Groth16.Make(C).prove` holds (SURVEY.md 8b "zk_set_devices(mask)", 8e) -------------
 * zk_set_devices(mask): bit d selects HIP device d; the library's device list becomes the selected devices in ascending order.
 * zk_set_device_list: the general form -- `count` device indices in the order given.  An index may appear MORE THAN ONCE ("virtual devices": several
 * shards of a key on one card, each with its own streams, tables and slots); that is how a one-GPU box exercises the multi-device path, it is never
 * faster than the plain list.  Both may be called before anything else or whenever no key handle is alive (ZK_ERR_ARG otherwise); zk_init(d) afterwards
 * succeeds iff d is the list's first entry.
 * With a list of N > 1 entries:
 *   - zk_groth16_pk_upload / _upload_lagrange shard the key over the list (slice g of both pools on entry g, cut by zk_groth16_shard_range for equal
 *     work) and return ONE handle; zk_groth16_prove / _prove_async / _prove_wait / _set_witness / _reserve_slots / _pk_derive_lagrange / _qap_eval /
 *     _pool_points / _pk_free work on it exactly as on a single-GPU key and produce the SAME bytes (groth16.ml:123-161: the proof does not depend on how
 *     the sums are cut).  Per proof: the Fr stage (QAP.eval, QAP.ml:120-135) runs once, on the slot's owner device (slot mod N); every device copies
 *     its slices of the three scalar vectors out of the owner's memory (hipMemcpyPeerAsync over xGMI), runs its part of the three multi-scalar
 *     products and sends 768 bytes of partial sums to the first device, which adds them and emits the proof.  Nothing blocks before _prove_wait.
 *   - zk_groth16_pk_derive_lagrange derives one of the three independent sets per device (devices 0, 1, 2 of the list) and installs every shard.
 *   - zk_pinocchio_pk_upload likewise cuts every one of the key's eight pools in N slices behind ONE handle (round 5); zk_pinocchio_prove / _prove_async /
 *     _prove_wait / _set_witness / _reserve_slots / _pk_derive_lagrange / _pool_points / _pk_free work on it as on a single-GPU key, same bytes: the Fr stage
 *     and the eight scalar vectors once on the slot's owner device, every device its slices of the eight products (pinocchio.ml:438-505), 1 920 bytes of
 *     partial sums to the first device, which adds them.  The consistency check behind the compact h pool and the derivation of the h bases run on the
 *     first device.
 *   - everything else (zk_msm_*, zk_fr_*, keygen helpers, verify, the explicit one-process-per-GPU shard API below) runs on the list's FIRST
 *     device; the shard API (zk_groth16_pk_upload_sharded, _prove_partial*, _scalars_async ...) refuses multi-device handles with ZK_ERR_ARG.
 * The one-process-per-GPU path (torch.distributed / RCCL, bench.py --gpus N) does not use the device list: every rank keeps its one-entry list. */
int zk_set_devices(uint64_t mask);
/* Configuration by call instead of by environment.  The reference configures by functor application (no flags, no environment), and an
 * OCaml host cannot change the process environment after the library was loaded in a way the C side is sure to see; the tuning knobs INTEGRATION.md 5
 * lists as environment variables are therefore also settable here: name = the variable's name, with or without the "ZK_" prefix, in either case
 * ("msm_window", "ZK_MSM_WINDOW"); value = the string the variable would hold; value == NULL hands the knob back to the environment.  An option set
 * here wins over the environment.  Knobs are read when a key is uploaded or at the first proof and cached: set options BEFORE the first key upload.
 * Unknown names -> ZK_ERR_ARG.  None changes a result (the one that changes a precondition, key_subgroup_check = 0, also switches off the folded
 * windows that rely on it).
 * ZK_GRAPH=1 captures each slot's proof once into a hipGraph and replays it, so the device pointers a proof reads are frozen at the first proof of the
 * slot.  Some of them point at tables that belong to the device, not to the key, and that grow when a later call needs more of them (a larger key
 * of either protocol, zk_fr_ntt or zk_fr_poly_mul at a larger size): the twiddle tables of the Fr stage.  The rule for those, with or without graphs:
 *   a device pointer to a table of the device, once handed to an enqueue or a capture, stays valid and keeps its values until zk_shutdown.
 * A table that grows is replaced for later calls and kept for earlier ones (each growth at least doubles it, so all old tables together cost less
 * than the current one); nothing is released before zk_shutdown.  Hence any call may be made while ANOTHER handle has proofs in flight or graphs
 * captured -- uploads, frees, zk_fr_*, zk_msm_*, key checks, verification; the restrictions stated with the single calls concern the slots of the
 * handle they are called on. */
int zk_set_option(const char* name, const char* value);
int zk_set_device_list(const int32_t* devices, uint32_t count);
int zk_get_device_list(int32_t* devices /* may be NULL */, uint32_t capacity, uint32_t* count);

/* ---- Fr stage ---------------------------------------------------------------------------
 * FFT.Make(F).fft / ifft over Bls12_381.Fr -- src/lib/zk/FFT.ml:29-86,222-233:
 * out[k] = sum_j a_j w_N^(jk), w_N = w^(2^32/N), w = 5^((r-1)/2^32); natural order in and out;
 * inverse uses w^-1 and divides by N.  inout: 2^log_n Fr elements. */
int zk_fr_ntt(uint8_t* inout, uint32_t log_n, int inverse);

/* FFT.Make(F).polynomial_mul -- src/lib/zk/FFT.ml:98-105 (== Polynomial.mul, polynomial.ml:124-131):
 * out receives na+nb-1 coefficients (low -> high), *nout the normalized length. */
int zk_fr_poly_mul(const uint8_t* a, size_t na, const uint8_t* b, size_t nb, uint8_t* out, size_t* nout);

/* ---- curve plugin seam (Curve.S.G, src/lib/zk/curve.mli:3-31) ------------------------------
 * G.apply_powers cs xis / G.dot m c -- src/lib/zk/curve.ml:94-118: sum_i scalars[i] * bases[i]
 * over the first nscalars bases.  nscalars > nbases -> ZK_ERR_APPLY_POWERS.  window_bits 0 = auto. */
int zk_msm_g1(const uint8_t* bases, size_t nbases, const uint8_t* scalars, size_t nscalars,
              uint32_t window_bits, uint8_t out[96]);
int zk_msm_g2(const uint8_t* bases, size_t nbases, const uint8_t* scalars, size_t nscalars,
              uint32_t window_bits, uint8_t out[192]);

/* ---- resident MSM bases: a point list uploaded once, multiplied many times ----------------------
 * The reference multiplies the SAME list again and again: sum_apply_powers calls G.apply_powers p ti once per variable with one ti
 * (src/groth16/groth16.ml:116-121), G.dot runs on the same key maps for every proof (curve.ml:94-103).  A handle keeps the list on the
 * device with its window tables, workspaces and staging buffers, so that a product costs one H2D copy, the launches and one D2H copy.
 *   group: 0 = G1 (96-byte points), 1 = G2 (192-byte points), the encodings of zk_msm_g1/g2.
 *   Upload checks every point as the key uploads do (of_bytes_exn, curve.ml:199-212): encoding (ZK_ERR_ARG), curve equation and [r] P = O
 *   (ZK_ERR_NOT_ON_CURVE); no handle then.  The identity, duplicates and P, -P pairs are allowed.  ZK_KEY_SUBGROUP_CHECK=0 skips the [r] P = O
 *   part as for keys (and the handle then never uses folded digits); the handle keeps the verdict of its upload.
 *   zk_msm_resident = G.apply_powers cs xis over the uploaded list (curve.ml:112-118): nscalars > n -> ZK_ERR_APPLY_POWERS (:116), nscalars = 0 ->
 *   the identity (:115), nscalars < n -> the first nscalars points; a scalar >= r -> ZK_ERR_SCALAR_RANGE (the handle stays usable).  The bytes
 *   are those of zk_msm_g1/g2 on the same prefix.
 *   zk_msm_resident_many: `count` such products over the same list; product k takes lens[k] scalars, concatenated in `scalars`; out: count
 *   points.  Any lens[k] > n -> ZK_ERR_APPLY_POWERS before anything runs; lens[k] = 0 -> the identity.
 *   Which path a product takes (the bytes are the same either way): when ONE call carries two or more products of 1 .. short_max scalars
 *   (zk_bases_info, per group), those run in two launches, a bucket kernel over a narrow window table and then the encoding; so does the
 *   only short product of a call when the list is long against it (length x 2048 < n in G1, x 4096 in G2).  Every other product -- longer
 *   than short_max, or alone on a shorter list, so most zk_msm_resident calls -- runs the Pippenger chain of zk_msm_g1/g2 over all n points
 *   of the handle (the scalars past the product's length are zero): its cost follows n, not the length.  Unknown or freed handle -> ZK_ERR_HANDLE.  The handle lives on the first device of the
 *   list at upload, is called from one host thread like the key handles, and counts as a live key handle for zk_set_devices /
 *   zk_set_device_list; zk_shutdown frees it. */
int zk_bases_upload(int group, const uint8_t* points, size_t n, uint64_t* handle);
int zk_bases_info(uint64_t handle, int* group, uint64_t* n, uint64_t* short_max);   /* any out may be NULL */
int zk_bases_free(uint64_t handle);
int zk_msm_resident(uint64_t handle, const uint8_t* scalars, size_t nscalars, uint8_t* out);
int zk_msm_resident_many(uint64_t handle, const uint8_t* scalars, const uint64_t* lens, uint32_t count, uint8_t* out);

/* G.of_Fr mapped over a vector (G1.one * s_i) -- src/lib/zk/curve.ml:180; the engine of
 * G.powers (curve.ml:106-109) and of keygen (groth16.ml:70-90, pinocchio.ml:104-156). */
int zk_g1_of_fr(const uint8_t* scalars, size_t n, uint8_t* out /* n*96 */);
int zk_g2_of_fr(const uint8_t* scalars, size_t n, uint8_t* out /* n*192 */);
/* G.powers d s = [ g^(s^i) | i = 0..d ] -- src/lib/zk/curve.ml:106-109 (d+1 points). */
int zk_g1_powers(uint32_t d, const uint8_t s[32], uint8_t* out /* (d+1)*96 */);
int zk_g2_powers(uint32_t d, const uint8_t s[32], uint8_t* out /* (d+1)*192 */);

/* to_compressed_bytes (curve.ml:199,208) of one uncompressed point. */
int zk_g1_compress(const uint8_t in[96], uint8_t out[48]);
/* of_compressed_bytes_exn (curve.ml:199-212): square root, sign from the flag, curve + subgroup checks (host code) */
int zk_g1_decompress(const uint8_t in[48], uint8_t out[96]);
int zk_g2_decompress(const uint8_t in[96], uint8_t out[192]);
int zk_g2_compress(const uint8_t in[192], uint8_t out[96]);
/* The same of_compressed_bytes_exn over a whole list ON THE GPU (round 5): the reference's JSON holds every key point compressed (groth16.ml:24-34,
 * pinocchio.ml:37-60 through curve.ml:199-219), and a 2^20-constraint key is five million square roots and subgroup checks -- half an hour of one
 * host core through the calls above, about a second here.  n points in, n uncompressed points out; ZK_ERR_ARG when some point's compression flag is
 * missing or a coordinate is >= p, ZK_ERR_NOT_ON_CURVE when some abscissa is not on the curve or some point lies outside the prime-order subgroup
 * (the verdicts of the one-point calls; with several bad points in a list, the encoding error is reported first). */
int zk_g1_decompress_batch(const uint8_t* in /* n*48 */, size_t n, uint8_t* out /* n*96 */);
int zk_g2_decompress_batch(const uint8_t* in /* n*96 */, size_t n, uint8_t* out /* n*192 */);

/* ---- protocol seam: Groth16.Make(C).prove (src/groth16/groth16.ml:235-237) -------------------
 * The circuit enters as sparse R1CS rows instead of the dense QAP.t (which is 3*m*n field
 * elements, QAP.ml:11-16): three CSR matrices L (`v`, left operand), R (`w`, right operand),
 * O (`y`, the gate's lhs) with n rows = gates in Gate.Set order (QAP.ml:22) and m columns =
 * variables in Var.compare order; `lhs = l * r` (src/lib/zk/circuit.ml:73-75). */
typedef struct {
    const uint32_t* row_ptr;   /* n + 1 */
    const uint32_t* col;       /* nnz   */
    const uint8_t* val;        /* nnz * 32, Fr */
} zk_csr;

/* One sparse matrix times one vector over Fr: y[g] = sum_e val[e] * x[col[e]] over row g.  With M = one R1CS matrix and x = the solution it gives the
 * VALUES at X = g of `eval' vps` (QAP.ml:121-131: sum_k sol_k poly_k evaluated at the gate's point); with M transposed and x = the Lagrange basis at tau
 * it gives every u_k(tau) of a keygen at once (groth16.ml:59-68, pinocchio.ml:104-109 -- `Poly.apply u_k s` per variable in the reference).
 * ZK_ERR_ARG for a malformed matrix (row_ptr not monotone, column >= cols), ZK_ERR_SCALAR_RANGE for a value >= r. */
int zk_fr_spmv(uint32_t rows, uint32_t cols, const zk_csr* M, const uint8_t* x /* cols * 32 */, uint8_t* y /* rows * 32 */);

/* The Lagrange basis of the QAP's integer points first .. first+n-1 (QAP.ml:84,92) at x: out[i] = l_i(x) = prod_{j != i} (x - first - j) / (i - j), i < n, and
 * z_out (may be NULL) = prod_j (x - first - j) -- what `Poly.apply` of the n interpolation polynomials and of the target gives (QAP.ml:84-100), for EVERY
 * x < r: the formula divides by nothing that depends on x, so at a point of the domain one value is 1, the others 0 and z = 0.  first = 0 is the
 * domain of v, w, y; first = n (with n - 1 points) that of the shifted points the Lagrange-form keys carry h on.  Canonical Fr bytes in and out.
 * ZK_ERR_ARG for n = 0, n > 2^24 or first + n > 2^32; ZK_ERR_SCALAR_RANGE for x >= r. */
int zk_fr_lagrange_at(uint32_t n, uint32_t first, const uint8_t x[32], uint8_t* out /* n*32 */, uint8_t z_out[32]);


/* Proving key of groth16.ml:24-34, fields in declaration order, plus the circuit.
 *   g1: a | d1 | b1 | ti1[n+2] | tiztd[n-1] | ltd_mid[n_mid]   (ltd_mid in Var.Map key order)
 *   g2: b2 | d2 | ti2[n+2]
 *   mid[k] != 0  <=>  variable k is in Dom(ltd_mid) (= circuit.mids, groth16.ml:74-79).
 * Uploads once, precomputes the per-n tables of the Fr stage, returns a handle.
 * KEY points (here, in the sharded / Lagrange-form uploads and in the Pinocchio upload) are checked the way the reference checks them on the way in
 * (of_bytes_exn / of_compressed_bytes_exn, curve.ml:199-212): canonical encoding (ZK_ERR_ARG), curve equation and membership of the prime-order
 * subgroup, [r] P = O on the device (both ZK_ERR_NOT_ON_CURVE; 0.3 s of a 2^20-constraint upload; ZK_KEY_SUBGROUP_CHECK=0 in the environment skips the
 * subgroup part for keys that were checked before).  The per-call bases of zk_msm_g1/g2 are checked for encoding and curve equation only and otherwise
 * TRUSTED to lie in G1 / G2, as every point an OCaml host obtained from Bls12_381.G1/G2 does.
 * The entry points that take points from outside -- zk_g1/g2_decompress, zk_pairing_*, zk_*_verify -- check the subgroup on the host. */
int zk_groth16_pk_upload(uint32_t n, uint32_t m, const zk_csr* L, const zk_csr* R, const zk_csr* O,
                         const uint8_t* mid /* m */, const uint8_t* pk_g1, size_t pk_g1_points,
                         const uint8_t* pk_g2, size_t pk_g2_points, uint64_t* handle);
/* Lagrange-form proving key (scope row f4 -- an EXTENSION of the key, only a keygen that knows tau can emit it;
 * keys in the reference's format use zk_groth16_pk_upload).  The tau-power lists are replaced by
 *   g1 = a | d1 | b1 | [l_i(tau)]_1 (n) | [lambda_t(tau) Z(tau)/delta]_1 (n-1) | ltd_mid        g2 = b2 | d2 | [l_i(tau)]_2 (n)
 * with l_i the Lagrange basis of the QAP's points 0..n-1 (QAP.ml:84,92) and lambda_t that of n..2n-2.  The same
 * group elements come out (proof bytes identical), but the prover needs only VALUES of v, w, h: three convolutions
 * instead of the O(n log^2 n) basis conversion.  All prove entry points work on the handle (zk_groth16_qap_eval still runs the
 * basis conversion: it is asked for coefficient vectors). */
int zk_groth16_pk_upload_lagrange(uint32_t n, uint32_t m, const zk_csr* L, const zk_csr* R, const zk_csr* O,
                                  const uint8_t* mid, const uint8_t* pk_g1, size_t pk_g1_points,
                                  const uint8_t* pk_g2, size_t pk_g2_points, uint64_t* handle);
/* Turns an uploaded key in the REFERENCE's format (tau powers, zk_groth16_pk_upload) into the Lagrange form above ON THE DEVICE and without
 * tau: [l_i(tau)] = V^-T [tau^k] is the transposed interpolation map applied to the key's own points (NTTs "in the exponent" over the
 * subproduct tree of the QAP's points, QAP.ml:84,92; csrc/lagrange_derive.hip).  O(n log^2 n) scalar multiplications ONCE per key
 * (seconds at 2^16 constraints, minutes at 2^20); afterwards every prove entry point runs the three-convolution Fr stage.  Proof bytes do
 * not change.  Single-GPU keys only; no proof may be in flight. */
int zk_groth16_pk_derive_lagrange(uint64_t handle);
/* The same in two halves, so that the N ranks of a node share ONE derivation instead of running it N times: the three derived sets -- bit 0:
 * [l_i(tau)]_1, bit 1: [l_i(tau)]_2, bit 2: the h bases [lambda_t(tau) Z(tau)/delta]_1 -- are independent of one another.  Every rank uploads the key
 * whole (zk_groth16_pk_upload), derives the sets of its `sets` mask into caller-owned DEVICE buffers holding the Lagrange-form pools
 * (zk_groth16_lagrange_pool_sizes points of 96 / 192 B; the copied parts a | d1 | b1, ltd_mid, b2 | d2 are always written, a set that is not
 * selected leaves its region untouched), the host framework broadcasts each set from its owner (RCCL broadcast on device memory: set 0 is
 * g1[3, 3+n), set 1 is g2[2, 2+n), set 2 is g1[3+n, 3+n+n-1)), and zk_groth16_pk_install_lagrange builds this rank's slice of the window tables
 * from the complete pools (world = 1: the whole key; same slicing rule as zk_groth16_pk_shard) and flips the key to the three-convolution
 * Fr stage.  zk_groth16_pk_derive_lagrange == _sets(handle, 7, ...) + _install(..., 0, 1).  The key is unchanged until _install has succeeded. */
int zk_groth16_lagrange_pool_sizes(uint64_t handle, uint64_t* g1_points, uint64_t* g2_points);
int zk_groth16_pk_derive_lagrange_sets(uint64_t handle, uint32_t sets, void* d_g1_out, void* d_g2_out);
int zk_groth16_pk_install_lagrange(uint64_t handle, const void* d_g1, const void* d_g2, uint32_t rank, uint32_t world);
/* Turns a key uploaded WHOLE (zk_groth16_pk_upload[_lagrange], possibly after zk_groth16_pk_derive_lagrange) into rank `rank`'s shard of a
 * point-sharded multi-GPU prover: the rank keeps its contiguous slice of both pools (same slicing rule as zk_groth16_pk_upload_sharded) and
 * from then on answers zk_groth16_prove_partial*.  How a derived Lagrange-form key reaches N GPUs: every rank uploads, derives, shards. */
int zk_groth16_pk_shard(uint64_t handle, uint32_t rank, uint32_t world);
/* ---- key generation in one call (a host that generates its own keys knows the trapdoor) ------------------------------------------------
 * Groth16 setup, groth16.ml:45-108: every exponent of the key is computed on the device from the trapdoor and the circuit (l_i(tau) as in
 * zk_fr_lagrange_at, the per-variable L_k(tau) of :59-68 through three transposed sparse products instead of one Poly.apply per variable), every
 * point comes from the fixed-base kernel (G.of_Fr, curve.ml:180).
 *   toxic = alpha | beta | gamma | delta | tau, the order Fr.gen is called (:51-55), canonical Fr bytes.
 *   pk_g1 / pk_g2 (each may be NULL): the key's bytes, ALWAYS in the reference's format -- tau powers, the layouts of zk_groth16_pk_upload, what
 *     pkey_to_yojson must see; *_points must be 3 + (n+2) + (n-1) + |mids| and 2 + (n+2) where the pointer is given (ZK_ERR_DOMAIN otherwise).
 *   vk_g1 = one1 | ltgm_io (1 + n_io points, Var order), vk_g2 = one2 | gm | d (groth16.ml:36-43; each may be NULL; ab = e(alpha, beta) is the caller's
 *     pairing of pk_g1[0] and pk_g2[0], :103).
 *   handle (may be NULL): a live key handle, as if the bytes had been uploaded -- `form` chooses what it holds: ZK_KEY_FORM_TAU_POWERS what
 *     zk_groth16_pk_upload would have built, ZK_KEY_FORM_LAGRANGE what upload + zk_groth16_pk_derive_lagrange would (same zk_groth16_pool_points
 *     bytes, every prove entry point works on it) in the time of a few fixed-base launches.  Bytes and handle come out of ONE pass over the same
 *     device exponents; the handle's base sets are built from the generated points where they lie (no host round trip, no decoding).  Generated
 *     points are multiples of the generator: ZK_KEY_SUBGROUP_CHECK does not apply to them.  zk_groth16_pk_free / zk_shutdown as for uploaded keys.
 * Status: ZK_ERR_ARG for a null L / R / O / mid / toxic, an unknown form, n outside [1, 2^24], m = 0, gamma = 0 or delta = 0 (the reference divides by
 * them, :70-90), a malformed matrix, and for handle != NULL while the device list has several entries (multi-device keygen is not offered; the
 * bytes can be had on any list, computed on its first device); ZK_ERR_DOMAIN for a wrong *_points; ZK_ERR_SCALAR_RANGE for a trapdoor scalar or a
 * matrix coefficient >= r; ZK_ERR_HIP without a GPU -- the argument checks (null, form, counts, trapdoor) come first.
 * Zero and degenerate trapdoors: alpha = 0, beta = 0 and tau = 0 are served like any value (a, b1, b2 are then the identity; the tau powers are
 * the generator followed by identities), and so is every other tau -- a point of the domain 0 .. n-1 (Z(tau) = 0: the l_i(tau) are a unit vector,
 * tiztd / hl all the identity), a point of n .. 2n-2 (the lambda_t(tau) are a unit vector), 1, r-1: l_i(tau) divides by nothing that depends on
 * tau.  Only gamma = 0 and delta = 0 are refused.  tests/test_gpu_degenerate_trapdoors.py holds each to the literal setup. */
#define ZK_KEY_FORM_TAU_POWERS 0
#define ZK_KEY_FORM_LAGRANGE   1
int zk_groth16_keygen(uint32_t n, uint32_t m, const zk_csr* L, const zk_csr* R, const zk_csr* O, const uint8_t* mid,
                      const uint8_t toxic[160], uint32_t form,
                      uint8_t* pk_g1, size_t pk_g1_points, uint8_t* pk_g2, size_t pk_g2_points,
                      uint8_t* vk_g1 /* (1 + n_io) * 96 */, uint8_t* vk_g2 /* 3 * 192 */, uint64_t* handle);
/* The key's resident base pool (group 1 or 2) as uncompressed points, in pool order: what was uploaded, or the derived Lagrange-form pool.
 * out == NULL: only *count. */
int zk_groth16_pool_points(uint64_t handle, int group, uint8_t* out, size_t capacity_points, size_t* count);
/* ---- keys and base lists in WIRE form: 48 B per G1 point, 96 B per G2 point ------------------------------------------------------------
 * Every key the reference writes holds its points compressed (to_compressed_bytes: groth16.ml:24-34, pinocchio.ml:37-60 through curve.ml:199-219).
 * The calls below take and give those bytes as they stand; the points are decoded ON THE DEVICE straight into the list the window tables are built
 * from -- one copy up at the compressed stride, the decompressor of zk_g1/g2_decompress_batch, the subgroup test, 8 bytes back -- instead of
 * zk_g1/g2_decompress_batch + zk_*_pk_upload (three trips over the bus per point, two subgroup tests).  Pool layouts, point counts and the
 * ZK_ERR_DOMAIN rules are those of the uncompressed calls; a handle made here cannot be told apart from one made there from the same points
 * (pool bytes, proof bytes, every prove / derive / shard entry point, zk_msm_resident*), on every device list on which those work: each device
 * decodes its own slice.
 *   Point checks (of_compressed_bytes_exn, curve.ml:199-212), the verdicts of zk_g1/g2_decompress_batch: compression flag missing, infinity bit on a
 *   string that is not C0 00 .. 00, coordinate >= p -> ZK_ERR_ARG; abscissa on no curve point, point outside the prime-order subgroup ->
 *   ZK_ERR_NOT_ON_CURVE.  The call returns the verdict of the FIRST bad point: the G1 list before the G2 list before h_lagrange.  No handle then.
 *   THE IDENTITY is C0 00 .. 00 and nothing else.  The all-zero string that the uncompressed uploads accept as the identity carries no compression
 *   flag: here it is a bad encoding (ZK_ERR_ARG).
 *   The subgroup test is the one by the curve's endomorphisms (2 x 63 doublings in G1, 63 in G2; the resident verification keys' test), the same
 *   answer as [r] P = O on every point of the curve.  ZK_KEY_SUBGROUP_CHECK=0 means what it means at upload: no subgroup test, no folded windows.
 *   Null L / R / O / mid / pools / handle or an unknown form -> ZK_ERR_ARG before the device is touched; without a GPU -> ZK_ERR_HIP.
 * zk_groth16_pk_upload_compressed: form = ZK_KEY_FORM_TAU_POWERS is zk_groth16_pk_upload, ZK_KEY_FORM_LAGRANGE is zk_groth16_pk_upload_lagrange (its
 *   lengths, and its caller's promise that the points are the key's Lagrange form -- which zk_groth16_key_check_lagrange puts to the test).
 * zk_pinocchio_pk_upload_compressed (below): h_lagrange = NULL is zk_pinocchio_pk_upload, else zk_pinocchio_pk_upload_lagrange (n points of 48 B;
 *   ZK_ERR_ARG under a device list of several entries, as there).  si[0] must be the generator's wire bytes.  The n + 1 G2 points between waw and the
 *   two appended points are not read, as in the uncompressed call.
 * zk_bases_upload_compressed: zk_bases_upload.
 * zk_*_pool_points_compressed: zk_*_pool_points (out == NULL / capacity / count alike) with every point as zk_g1/g2_compress gives it, the identity as
 *   C0 00 .. 00.  With the uploads it is the key-cache round trip: derive once (zk_*_pk_derive_lagrange), store the compressed pools, later load them
 *   with form = ZK_KEY_FORM_LAGRANGE (Groth16: both pools) / h_lagrange (Pinocchio: the first n points of pool 5).
 * Measured on one MI355X, host wall time from the compressed bytes to a handle that has produced one oracle-equal proof, best of five, the two routes
 * alternating (profiles/key_load_compressed.json): Groth16 2^20 (4.19 M points) 0.693 s against 1.804 s for zk_g1/g2_decompress_batch x 2 +
 * zk_groth16_pk_upload (spread of that route's five timings 0.022 s), 0.505 s under ZK_KEY_SUBGROUP_CHECK=0; Groth16 2^16 82 ms against 190 ms
 * (spread 8 ms); Pinocchio 2^18 0.498 s against 1.321 s (spread 0.017 s).  Device time at 2^20 by family (zk_profile_get): key_decompress 46 ms,
 * subgroup_check 180 ms, msm_precompute 374 ms.  zk_groth16_pool_points_compressed at 2^20: 87 ms, against 486 ms for zk_groth16_pool_points + host
 * compression.  Kernels (profiles/key_wire_kernel_resources.txt; no spills): k_decompress 108 / 178 VGPRs and 80 / 144 B of scratch per lane (G1 / G2),
 * k_subgroup_check by endomorphism 248 / 256 VGPRs and 1168 / 1872 B, k_compress 84 / 128 VGPRs and no scratch.  Timer families: key_decompress,
 * key_compress; the subgroup launch stays in subgroup_check. */
int zk_groth16_pk_upload_compressed(uint32_t n, uint32_t m, const zk_csr* L, const zk_csr* R, const zk_csr* O, const uint8_t* mid,
                                    const uint8_t* pk_g1 /* points * 48 */, size_t pk_g1_points,
                                    const uint8_t* pk_g2 /* points * 96 */, size_t pk_g2_points,
                                    uint32_t form /* ZK_KEY_FORM_TAU_POWERS | ZK_KEY_FORM_LAGRANGE */, uint64_t* handle);
int zk_bases_upload_compressed(int group, const uint8_t* points, size_t n, uint64_t* handle);
int zk_groth16_pool_points_compressed(uint64_t handle, int group, uint8_t* out, size_t capacity_points, size_t* count);
/* ---- the key as a whole: is this proving key a Groth16 key of THIS circuit, and the partner of this verification key? ---------------------
 * The uploads check a key point by point (encoding, curve, subgroup).  They do not check that ti1 / ti2 hold consecutive powers of one tau, that
 * tiztd and ltd_mid belong to the circuit and to the delta of d1 / d2, or that the proofs will verify under the verification key at hand.  A key
 * that fails one of these produces proofs that fail downstream; a CRAFTED ltd_mid or tiztd can make the proof element C leak witness values (Groth16
 * hides the witness only under a well-formed CRS).  zk_groth16_key_check tests every relation of groth16.ml:45-108 on the key that lies in the
 * handle, each as ONE random linear combination over all its indices.  With g1 = ti1[0], g2 = ti2[0] and pseudo-random rho, sigma, mu:
 *   ZK_KEYCHK_GENERATORS  ti1[0], ti2[0] (and the verification key's one1, one2) are the generators                         byte comparison
 *   ZK_KEYCHK_TAU_G1      ti1[i+1] = tau ti1[i], i <= n, tau that of ti2[1]      e(sum rho_i ti1[i+1], g2) = e(sum rho_i ti1[i], ti2[1])
 *   ZK_KEYCHK_TAU_G2      ti2[i] has the exponent of ti1[i], i <= n+1            e(sum rho_i ti1[i], g2) = e(g1, sum rho_i ti2[i])
 *   ZK_KEYCHK_BETA        b1, b2 hold one beta                                   e(b1, g2) = e(g1, b2)
 *   ZK_KEYCHK_DELTA       d1, d2 hold one delta, delta != 0, vk.d = d2           e(d1, g2) = e(g1, d2); identity test; byte comparison
 *   ZK_KEYCHK_H_BASES     tiztd[i] delta = tau^i Z(tau), i < n-1                 e(sum sigma_i tiztd[i], d2) = e(sum sigma_i ti1[i], <ti2, coefficients of Z>)
 *   ZK_KEYCHK_L           ltd_mid[k] delta = L_k(tau) for k in mids, and with a verification key ltgm_io[k] gamma = L_k(tau) for the others (:59-99)
 *                         e(sum mu_k ltd_mid[k], d2) e(sum mu_k ltgm_io[k], gm) = e(V, b2) e(a, W) e(Y, g2),  V = <ti1, coefficients of sum mu_k v_k>,
 *                         W = <ti2, .. w_k>, Y = <ti1, .. y_k>; without a verification key mu is 0 outside mids and the gm pair drops out
 *   ZK_KEYCHK_GAMMA       gamma != 0 (verification key only)                     identity test
 * A relation reads other points of the key: a wrong ti2[1] also trips ZK_KEYCHK_H_BASES.  The sums are products over the handle's own window tables
 * (eight in G1, three in G2: the work of about four proofs), the coefficient vectors come from the prover's Fr stage with mu in the witness's place,
 * the pairings run on the device (the kernels of zk_pairing_product_many, without its point checks: every point is checked already).  vk.ab is not an argument: its bytes are the caller's pairing of pk_g1[0] and pk_g2[0].
 *   handle: a tau-power key held whole on one device (zk_groth16_pk_upload, zk_groth16_pk_upload_compressed or zk_groth16_keygen with
 *     ZK_KEY_FORM_TAU_POWERS).  The call leaves it as it found it: a proof made after the check has the bytes of one made before.
 *   vk_g1 = one1 | ltgm_io (1 + n_io points), vk_g2 = one2 | gm | d: the layouts zk_groth16_keygen writes; both or neither.  n_io = m - |mids|.
 *   THE CONTRACT FOR seed is that of rho in zk_groth16_verify_folded: 32 bytes from a cryptographic generator, drawn AFTER the key's bytes are fixed
 *     and unpredictable to whoever made the key.  A malformed key then passes a relation with probability below 2^-253; with the seed known in advance
 *     a key CAN be built whose defects cancel under the coefficients it expands to.  NULL: the library draws the bytes (std::random_device).  All 256
 *     bits reach the coefficients: each 64-bit limb of every coefficient is a stream of its own, keyed by 8 bytes of the seed.  The verdict on a
 *     well-formed key does not depend on the seed.
 *   Returns ZK_OK whenever the check ran; *failed is the mask of the relations that do not hold, 0 for a well-formed key.  A malformed key is a
 *     verdict, not an error.  Refused before the device is touched, with ZK_ERR_ARG: failed null; exactly one of vk_g1 / vk_g2; an n_io that is not
 *     m - |mids|; a handle in Lagrange form (zk_groth16_key_check_lagrange checks that form); a shard or a multi-device handle; a handle with a
 *     proof in flight; a handle uploaded under ZK_KEY_SUBGROUP_CHECK=0 (pairing relations mean nothing outside the subgroup, and the check does not
 *     repeat the upload's work).  An unknown handle -> ZK_ERR_HANDLE (without a GPU: ZK_ERR_HIP, no handle can exist).  The verification key's points
 *     are decoded and checked like those of zk_groth16_vk_upload, with its codes.
 *   Out of scope: Pinocchio keys; sharded and multi-device handles (those three still rest on their caller's promise); Lagrange-form handles have
 *     the call below; no upload checks anything more by default.  Timer family of the check's own launches: key_check. */
#define ZK_KEYCHK_GENERATORS 1u
#define ZK_KEYCHK_TAU_G1     2u
#define ZK_KEYCHK_TAU_G2     4u
#define ZK_KEYCHK_BETA       8u
#define ZK_KEYCHK_DELTA      16u
#define ZK_KEYCHK_H_BASES    32u
#define ZK_KEYCHK_L          64u
#define ZK_KEYCHK_GAMMA      128u
int zk_groth16_key_check(uint64_t handle, const uint8_t* vk_g1 /* one1 | ltgm_io, may be NULL */, size_t n_io,
                         const uint8_t* vk_g2 /* one2 | gm | d, may be NULL */,
                         const uint8_t seed[32] /* may be NULL */, uint32_t* failed /* bit mask, 0 = well formed */);
/* ---- a Lagrange-form key as a whole -----------------------------------------------------------------------------------------------------------
 * The same question for a handle in Lagrange form, however it came by it: zk_groth16_pk_upload_lagrange, zk_groth16_pk_upload_compressed or
 * zk_groth16_keygen with ZK_KEY_FORM_LAGRANGE, zk_groth16_pk_derive_lagrange.  Pools read back from a key cache are bytes from somewhere else: this is
 * the check between loading them and proving, without the derivation the cache exists to save.  Such a handle holds no tau power, not even [tau]_2, so
 * the relations are stated on VALUES.  Pools g1 = a | d1 | b1 | l1[n] | hl[n-1] | ltd_mid, g2 = b2 | d2 | l2[n]; l_i the Lagrange basis of the points
 * 0..n-1, lambda_t of n..2n-2, w_i = (-1)^(n-1-i) / (i! (n-1-i)!) the barycentric weights of 0..n-1; g1 := sum l1[i], g2 := sum l2[i] (honestly the
 * generators: sum l_i = 1), T2 := sum i l2[i] (honestly [tau]_2: sum i l_i(X) = X for n >= 2).  The bits are those of zk_groth16_key_check:
 *   ZK_KEYCHK_GENERATORS  sum l1 = [1]_1, sum l2 = [1]_2 (and the verification key's one1, one2 are the generators)          byte comparison
 *   ZK_KEYCHK_TAU_G2      l1[i] g2 = g1 l2[i]                                     e(sum rho_i l1[i], g2) = e(g1, sum rho_i l2[i])
 *   ZK_KEYCHK_TAU_G1      l1 is the Lagrange basis at ONE point: l1[i] (i g2 - T2) is proportional to w_i (n >= 2)
 *                         e(sum i pi_i l1[i], g2) = e(sum pi_i l1[i], T2) for pi in the hyperplane sum w_i pi_i = 0 -- the values on 0..n-1 of a polynomial
 *                         q of degree <= n-2; a linear form vanishes on all of it exactly when its coefficients are proportional to w
 *   ZK_KEYCHK_BETA        b1 g2 = g1 b2                                           e(b1, g2) = e(g1, b2)
 *   ZK_KEYCHK_DELTA       d1 g2 = g1 d2, delta != 0, vk.d = d2                    e(d1, g2) = e(g1, d2); identity test; byte comparison
 *   ZK_KEYCHK_H_BASES     w_0 hl[t] d2 = l2[0] sum_i i lambda_t(i) l1[i], t < n-1, i.e. hl[t] delta = lambda_t(tau) Z(tau) (tau l_0(tau) / w_0 = Z(tau))
 *                         e(sum_t w_0 sigma_t hl[t], d2) = e(S, l2[0]), sigma_t = q(n + t), S = sum i pi_i l1[i] (the sum TAU_G1 has made); pi -> sigma is a
 *                         bijection onto Fr^(n-1), so every t has a coefficient of its own
 *   ZK_KEYCHK_L           ltd_mid[k] d2 (mids; with a verification key ltgm_io[k] gm for the others) = (sum_i L[i,k] l1[i]) b2 + a (sum_i R[i,k] l2[i])
 *                         + (sum_i O[i,k] l1[i]) g2:   e(sum mu_k ltd_mid[k], d2) e(sum mu_k ltgm_io[k], gm) = e(V, b2) e(a, W) e(Y, g2),
 *                         V = sum_i (L mu)_i l1[i], W = sum_i (R mu)_i l2[i], Y = sum_i (O mu)_i l1[i]
 *   ZK_KEYCHK_GAMMA       gamma != 0 (verification key only)                      identity test
 * For n = 1 TAU_G1 and H_BASES are vacuous and never set.  A well-formed basis of ANOTHER point (the tau of hl and ltd_mid shifted, or the domain 1..n,
 * which is the domain 0..n-1 at tau - 1) passes TAU_G1 and fails H_BASES and L.  No basis conversion runs: pi comes from a raw vector without a
 * division, sigma by the prover's own extrapolation, L mu | R mu | O mu from its Fr stage with mu in the witness's place; twelve products over the
 * handle's window tables (eight in G1, four in G2), twelve pairing products on the device.
 *   handle: a Lagrange-form key held whole on one device.  Nothing of the handle is written: a proof made after the check has the bytes of one made
 *     before.  vk_g1, n_io, vk_g2, seed (THE SAME CONTRACT), the return value ("a malformed key is a verdict, not an error"), the decoding of the
 *     verification key with its codes and the timer family key_check are those of zk_groth16_key_check.
 *   Refused before the device is touched, with ZK_ERR_ARG: failed null; exactly one of vk_g1 / vk_g2; an n_io that is not m - |mids|; a tau-power
 *     handle (zk_groth16_key_check is its call); a shard or a multi-device handle; a handle with a proof in flight; a handle made under
 *     ZK_KEY_SUBGROUP_CHECK=0.  An unknown handle -> ZK_ERR_HANDLE (without a GPU: ZK_ERR_HIP). */
int zk_groth16_key_check_lagrange(uint64_t handle, const uint8_t* vk_g1 /* one1 | ltgm_io, may be NULL */, size_t n_io,
                                  const uint8_t* vk_g2 /* one2 | gm | d, may be NULL */,
                                  const uint8_t seed[32] /* may be NULL */, uint32_t* failed /* bit mask, 0 = well formed */);
/* ---- a delta contribution to a resident key ----------------------------------------------------------------------------------------------------
 * The checks above tell a host that a key is well formed; they cannot tell it that whoever made the key has forgotten delta.  The usual remedy is a
 * phase-2 contribution: a party multiplies delta by a secret delta', and the key is sound if ONE party forgets its factor.  Of a key (groth16.ml:45-108)
 * only d1, d2 (delta), tiztd[i] or hl[t], ltd_mid[k] (1 / delta) and vkey.d (= d2) depend on delta.  This call changes, in place on the device:
 *   g1[1] = d1 and g2[1] = d2    <- delta' times the point
 *   the tail of the G1 pool       <- 1 / delta' mod r times every point:  tiztd[n-1] | ltd_mid[|mids|], in Lagrange form hl[n-1] | ltd_mid
 * and nothing else.  The window tables of both pools are built again from the points on the device, the way zk_groth16_keygen and
 * zk_groth16_pk_install_lagrange build them: no host round trip, no decoding, no subgroup test -- a multiple of a subgroup point is in the subgroup; a
 * ZK_KEY_SUBGROUP_CHECK=0 origin is inherited as it stands.  The identity stays the identity.  The handle is unchanged until the new pools and tables
 * are complete; then they replace the old ones, and every slot of the handle (its workspaces, under ZK_GRAPH its captured proofs) is dropped and built
 * again at its next use: a proof on a slot used before the call comes out under the NEW key.  Afterwards the handle cannot be told apart from one
 * uploaded from the contributed key's bytes: pool bytes, proofs on every entry point, a later derivation, both key checks, zk_groth16_pk_shard.
 *   dmul: delta', canonical Fr bytes.  link_g1: d1 before | d1 after.  dmul_g2: [delta']_2.  vk_d: d2 after, the d of the new verification key (ab and
 *     ltgm_io do not depend on delta).  A link shows e(d1 after, g2) = e(d1 before, [delta']_2): the RATIO of two delta.  A ceremony's transcript hash
 *     and its proof of knowledge of delta' are the caller's protocol.
 *   Before the device is touched: null dmul -> ZK_ERR_ARG; delta' = 0 -> ZK_ERR_ARG (the reference divides by delta); delta' >= r ->
 *     ZK_ERR_SCALAR_RANGE.  An unknown or freed handle, a Pinocchio handle -> ZK_ERR_HANDLE (without a GPU: ZK_ERR_HIP).  A shard, a multi-device
 *     handle, a handle with a proof in flight -> ZK_ERR_ARG.  After any refusal the handle proves exactly as before.
 * The multiplications run on the kernels of the Lagrange derivation (csrc/lagrange_derive.hip: k_aff_to_raw, k_g_tabmul, k_raw_to_aff) over a table of
 * equal scalars (csrc/contribute.hip); a kernel of its own was built, measured against them and dropped (profiles/contribute_kernel_ab.json).
 * Timer family contribute. */
int zk_groth16_pk_contribute(uint64_t handle, const uint8_t dmul[32] /* delta', canonical Fr bytes */,
                             uint8_t link_g1[2 * 96]   /* d1 before | d1 after, may be NULL */,
                             uint8_t dmul_g2[192]      /* [delta']_2, may be NULL */,
                             uint8_t vk_d[192]         /* d2 after = the new vkey.d, may be NULL */);
/* ---- a phase-1 string specialised to a circuit ---------------------------------------------------------------------------------------------------
 * The deterministic station between a powers-of-tau string and phase 2: from [tau^i]_1, [alpha tau^i]_1, [beta tau^i]_1, [beta]_2, [tau^i]_2 and the
 * circuit, the key of groth16.ml:45-108 for the trapdoor (alpha, beta, gamma = 1, delta = 1, tau), byte for byte -- with no secret anywhere: every
 * point of the key is a linear combination of the string's points.  After it zk_groth16_pk_contribute moves delta and zk_groth16_key_check judges the
 * result; the trapdoor never exists on any host.
 *   srs_g1 = tau1[max(n+2, 2n-1)] | alpha_tau1[n] | beta_tau1[n]  (96 B each),  srs_g2 = beta2 | tau2[n+2]  (192 B each): uncompressed points, exactly
 *     the counts zk_groth16_srs_sizes gives (ZK_ERR_DOMAIN otherwise).
 *   Key bytes (pk_g1 / pk_g2 / vk_g1 / vk_g2 / handle / form: layouts, optionality and meaning as in zk_groth16_keygen):
 *     a = alpha_tau1[0]   d1 = the G1 generator   b1 = beta_tau1[0]   ti1 = tau1[0 .. n+1]   b2 = beta2   d2 = the G2 generator   ti2 = tau2
 *     tiztd[i] = sum_j z_j tau1[i+j], i < n-1, z the coefficients of Z = prod_{i<n} (X - i)        (one correlation in the exponent)
 *     ltd_mid[k] = sum_i (L[i,k] [beta l_i] + R[i,k] [alpha l_i] + O[i,k] [l_i]) for the mids, Var order (groth16.ml:59-68: beta with L, alpha with R);
 *       [l_i], [alpha l_i], [beta l_i] are derived from the three G1 lists as zk_groth16_pk_derive_lagrange derives [l_i] from ti1
 *     vk_g1 = one1 | ltgm_io (the same sum for the other variables, gamma = 1),  vk_g2 = one2 | gm | d: three times the G2 generator;
 *       ab = e(a, b2) stays the caller's pairing
 *   handle: what an upload of those bytes would build (ZK_KEY_FORM_TAU_POWERS), or that plus zk_groth16_pk_derive_lagrange (ZK_KEY_FORM_LAGRANGE;
 *     the [l_i]_1 of the specialisation are reused).  Every later call works on it: pool points, every prove entry point, contribute, both key checks.
 * The string's points come from outside and are checked like the points of zk_groth16_pk_upload, list by list in the order above, the first bad list
 * deciding: an encoding -> ZK_ERR_ARG, a point off the curve or outside the subgroup -> ZK_ERR_NOT_ON_CURVE.  ZK_KEY_SUBGROUP_CHECK=0 skips the
 * subgroup part, and the handle remembers it: zk_groth16_key_check refuses it as it refuses such uploads.
 * TRUST: the call cannot know whether the string is well formed and does not try.  Whatever points it is given, the output is the linear map above
 * applied to them.  The contract is: run zk_groth16_key_check (or zk_groth16_key_check_lagrange) with the returned verification key on the result.
 * A string whose lists disagree gives a key that fails it (alpha_tau1 not alpha tau^i: bit L; a wrong high power of tau1: bit H_BASES).  The check of
 * the string itself -- the powers beyond n+1, the alpha and beta lists against tau2 -- is zk_groth16_srs_check below: run it once on the whole string.
 * Status, in this order, everything before ZK_ERR_HIP without touching the device: ZK_ERR_ARG for a null L / R / O / mid / srs_g1 / srs_g2, an unknown
 * form, n outside [1, 2^24] (the transforms in the exponent run at 2 * 2^ceil(log2 n) <= 2^25 points, the bound of zk_groth16_keygen and of the
 * derivation) or m = 0; ZK_ERR_DOMAIN for any *_points that is not exactly the expected count; ZK_ERR_ARG for a malformed matrix or more than
 * 2^30 - 1 variables plus nonzero entries; ZK_ERR_SCALAR_RANGE for a matrix coefficient >= r; ZK_ERR_HIP without a GPU; ZK_ERR_ARG for handle != NULL
 * while the device list has several entries; then the verdict on the string.  A refused call writes nothing and leaves no handle.
 * Timer families specialize_derive, specialize_correlate, specialize_mul, specialize_sum (and lagrange_derive for the Lagrange-form handle). */
int zk_groth16_srs_sizes(uint32_t n, uint64_t* tau_g1, uint64_t* ab_g1, uint64_t* tau_g2);          /* max(n+2, 2n-1), n, n+2; each may be NULL */
int zk_groth16_pk_specialize(uint32_t n, uint32_t m, const zk_csr* L, const zk_csr* R, const zk_csr* O, const uint8_t* mid,
                             const uint8_t* srs_g1, size_t srs_g1_points, const uint8_t* srs_g2, size_t srs_g2_points, uint32_t form,
                             uint8_t* pk_g1, size_t pk_g1_points, uint8_t* pk_g2, size_t pk_g2_points,
                             uint8_t* vk_g1 /* (1 + n_io) * 96 */, uint8_t* vk_g2 /* 3 * 192 */, uint64_t* handle);
/* ---- a phase-1 string as a whole: the check and a contribution ------------------------------------------------------------------------------------
 * The two stations BEFORE zk_groth16_pk_specialize.  A string has the lists and layout of that call -- srs_g1 = tau1[N1] | alpha_tau1[NAB] |
 * beta_tau1[NAB] (96 B each), srs_g2 = beta2 | tau2[N2] (192 B each), uncompressed -- but its lengths are the caller's, not a circuit's: one long string
 * is checked once and then cut to many circuits.  N1 >= 2, N2 >= 2, NAB >= 1; NAB <= N1 and N2 <= N1 (BETA and TAU_G2 compare against tau1[i]);
 * N1 <= 2^25 (what zk_groth16_srs_sizes gives at n = 2^24).
 *
 * zk_groth16_srs_check: is this a well-formed string of SOME trapdoor (alpha, beta, tau)?  Each of the four relations is one equation between two
 * pairing products; the sums run over all its indices with coefficients rho_i expanded from the seed (the generator and the seed contract of
 * zk_groth16_key_check: 32 bytes drawn AFTER the string's bytes are fixed, unpredictable to whoever made it; NULL: drawn here).  g1, g2 the generators:
 *   ZK_SRSCHK_GENERATORS  tau1[0] = g1, tau2[0] = g2                                                  byte comparison
 *   ZK_SRSCHK_TAU_G1      tau1[i+1] = tau tau1[i], i < N1-1, tau the exponent of tau2[1]              e(sum rho_i tau1[i+1], g2) = e(sum rho_i tau1[i], tau2[1])
 *   ZK_SRSCHK_TAU_G2      tau2[i] holds the exponent of tau1[i], i < N2                               e(sum rho_i tau1[i], g2) = e(g1, sum rho_i tau2[i])
 *   ZK_SRSCHK_ALPHA       alpha_tau1[i+1] = tau alpha_tau1[i], i < NAB-1                              the form of TAU_G1 over alpha_tau1
 *   ZK_SRSCHK_BETA        beta_tau1[i] = beta tau1[i], i < NAB, beta the exponent of beta2            e(sum rho_i beta_tau1[i], g2) = e(sum rho_i tau1[i], beta2)
 *   ZK_SRSCHK_TRIVIAL     tau2[1], alpha_tau1[0] or beta2 is the identity: a component of the trapdoor is 0          identity test
 * A relation with no index holds (ALPHA at NAB = 1); a sum over fewer than N1 points of tau1 is the long sum with zero coefficients.  A relation that
 * fails at one index fails the check with probability 1 - 1/r.  A malformed string is a VERDICT: ZK_OK and a non-zero mask.  A bad POINT is a
 * status: the lists are decoded in the order tau1, alpha_tau1, beta_tau1, beta2 | tau2, the first bad list decides, with the codes of
 * zk_groth16_pk_specialize (encoding -> ZK_ERR_ARG, off the curve or outside the subgroup -> ZK_ERR_NOT_ON_CURVE).  The subgroup test ALWAYS runs, by
 * the curves' endomorphisms, whatever ZK_KEY_SUBGROUP_CHECK says: a pairing does not see a cofactor component, so a check that skipped the test would
 * vouch for points it had not looked at.  Zero bytes are the identity, as in every key list.
 * Status, in this order, everything before ZK_ERR_HIP without touching the device: ZK_ERR_ARG for a null srs_g1 / srs_g2 / failed or a count below
 * its minimum; ZK_ERR_DOMAIN for NAB > N1, N2 > N1, N1 > 2^25; ZK_ERR_HIP without a GPU; ZK_ERR_ARG on a device list of several entries; then the
 * points.  A refused call leaves *failed as it was.  No state outlives the call.  The sums are Pippenger products over base sets built for the call
 * WITHOUT window tables (a string is multiplied once; DESIGN 2t, profiles/srs_ab.json); the four sums over tau1 share one chain of sort and
 * accumulate launches, the two over alpha_tau1 another.  Timer family srs_check (stages srs_check:decode, :subgroup, :sums, :pairings).
 * One MI355X, the string of a circuit of n constraints (profiles/srs.json): 60 ms at n = 2^16, 125 ms at 2^18, 328 ms at 2^20; with tables the call
 * at 2^18 takes 223 ms instead of 123 ms (profiles/srs_ab.json).
 *
 * zk_groth16_srs_contribute: the string times (alpha', beta', tau') on the device -- the step that makes a string trustworthy if ONE contributor
 * forgets its factors:
 *   tau1[i] tau'^i     alpha_tau1[i] alpha' tau'^i     beta_tau1[i] beta' tau'^i     beta2 beta'     tau2[i] tau'^i
 * The identity stays the identity.  The call TRUSTS the string as zk_groth16_pk_specialize does: it applies a linear map and does not repair a
 * malformed string (check before and after).  The points are checked like those of zk_groth16_pk_specialize; ZK_KEY_SUBGROUP_CHECK=0 is honoured
 * here.  mul: alpha' | beta' | tau', canonical Fr bytes, the order SRS.generate draws a trapdoor in.  out_g1 / out_g2: the layouts of the inputs; each
 * may be its input's own memory.  link_g1 = tau1[1] before | after, alpha_tau1[0] before | after, beta_tau1[0] before | after; link_g2 = [tau']_2 |
 * [alpha']_2 | [beta']_2: three RATIOS, each shown by e(after, g2) = e(before, [x']_2).  The proof of knowledge of the factors and the transcript are
 * the ceremony's, as for zk_groth16_pk_contribute.
 * Status, in this order, before the device is touched: ZK_ERR_ARG for a null srs_g1 / srs_g2 / mul / out_g1 / out_g2 or a count below its minimum;
 * ZK_ERR_DOMAIN for the lengths as above; a factor of 0 -> ZK_ERR_ARG, a factor >= r -> ZK_ERR_SCALAR_RANGE (the first bad factor in mul's order
 * decides).  Then ZK_ERR_HIP, the device list, the points.  A refused call writes nothing.  The scalars come from the power scan of
 * zk_groth16_keygen, the multiplications run on the kernels of zk_groth16_pk_contribute (points_scale_tabmul, both curves), [x']_2 on the fixed-base
 * kernel; the call has no kernel of its own.  Timer family srs_contribute (stages srs_contribute:scalars, :multiply). */
#define ZK_SRSCHK_GENERATORS 1u   /* tau1[0] is not the G1 generator or tau2[0] is not the G2 generator */
#define ZK_SRSCHK_TAU_G1     2u   /* some i < N1-1:  tau1[i+1] != tau * tau1[i],  tau the exponent of tau2[1] */
#define ZK_SRSCHK_TAU_G2     4u   /* some i < N2:    tau2[i] does not hold the exponent of tau1[i] */
#define ZK_SRSCHK_ALPHA      8u   /* some i < NAB-1: alpha_tau1[i+1] != tau * alpha_tau1[i] */
#define ZK_SRSCHK_BETA       16u  /* some i < NAB:   beta_tau1[i] != beta * tau1[i],  beta the exponent of beta2 */
#define ZK_SRSCHK_TRIVIAL    32u  /* tau2[1], alpha_tau1[0] or beta2 is the identity: a component of the trapdoor is 0 */
int zk_groth16_srs_check(const uint8_t* srs_g1, size_t tau1_points, size_t ab_points,
                         const uint8_t* srs_g2, size_t tau2_points,
                         const uint8_t seed[32] /* may be NULL: drawn here */, uint32_t* failed);
int zk_groth16_srs_contribute(const uint8_t* srs_g1, size_t tau1_points, size_t ab_points,
                              const uint8_t* srs_g2, size_t tau2_points,
                              const uint8_t mul[96]  /* alpha' | beta' | tau', canonical Fr: the order SRS.generate draws */,
                              uint8_t* out_g1, uint8_t* out_g2   /* same layouts; each may alias its input */,
                              uint8_t link_g1[6 * 96]  /* tau1[1], alpha_tau1[0], beta_tau1[0]: before | after each; may be NULL */,
                              uint8_t link_g2[3 * 192] /* [tau']_2 | [alpha']_2 | [beta']_2; may be NULL */);
int zk_groth16_pk_free(uint64_t handle);

/* Groth16.prove rng qap pkey sol with r, s supplied by the caller in the order the reference
 * draws them (groth16.ml:124-125; Fr.gen is an external function).
 * sol: m Fr values in Var.compare order (the witness incl. ONE).
 * proof: a (G1 96 B) | b (G2 192 B) | c (G1 96 B) uncompressed; zk_g*_compress gives the JSON form.
 * Returns ZK_ERR_REMAINDER when the witness does not satisfy the gates (QAP.ml:134). */
int zk_groth16_prove(uint64_t handle, const uint8_t* sol, const uint8_t r[32], const uint8_t s[32],
                     uint8_t proof[384]);
/* Pipelined form: up to 15 proofs in flight on one key, each on its own `slot` (own scratch and
 * HIP streams).  _async enqueues and returns; _wait blocks for that slot and delivers the proof.
 * The single-wave tails of one proof (bucket reduction, affine conversion) then run under the
 * bulk kernels of the next.  zk_groth16_prove == _async + _wait on slot 0. */
int zk_groth16_reserve_slots(uint64_t handle, uint32_t count);   /* allocate slots 0..count-1 now instead of at first use */
int zk_groth16_prove_async(uint64_t handle, const uint8_t* sol, const uint8_t r[32], const uint8_t s[32], uint32_t slot);
int zk_groth16_prove_wait(uint64_t handle, uint32_t slot, uint8_t proof[384]);
/* Keeps a witness resident in HBM; a later zk_groth16_prove / _prove_partial / _qap_eval called with
 * sol = NULL uses it (no host -> device copy inside the call). */
int zk_groth16_set_witness(uint64_t handle, const uint8_t* sol);

/* QAP.eval (src/lib/zk/QAP.ml:120-135) on the uploaded circuit: coefficient vectors of
 * v = sum_k sol_k v_k, w, and h = (v*w - y)/Z, each padded with zeros to n (h: n-1). Any out
 * pointer may be NULL. */
int zk_groth16_qap_eval(uint64_t handle, const uint8_t* sol, uint8_t* v_out, uint8_t* w_out, uint8_t* h_out);

/* ---- point-sharded multi-GPU prove --------------------------------------------
 * One process per GPU.  Rank `rank` of `world` uploads the same key but keeps only its contiguous
 * slice of the two base pools (g1: a | d1 | b1 | ti1 | tiztd | ltd_mid, g2: b2 | d2 | ti2); the Fr
 * stage is replicated.  zk_groth16_prove_partial returns the rank's partial sums of the three
 * multi-scalar products as raw XYZZ Montgomery limbs: A | C (G1, 4*48 B each) | B (G2, 4*96 B).
 * EC addition is not a reduction operator of RCCL, so the host all-gathers the `world` blocks as
 * bytes (torch.distributed / ncclAllGather over xGMI) and zk_groth16_combine adds them on the
 * GPU and emits the proof.  The sum is exact: the proof bytes do not depend on `world`.
 * The slices are cut for equal WORK, not equal length: the first 3 + (n+2 | n) points of the G1 pool
 * (a | d1 | b1 | the tau basis) carry two products of a proof (A and C: groth16.ml:128-134, :147-160),
 * the others one, so rank g holds [cut(g), cut(g+1)) with cut at equal shares of points + heavy prefix;
 * the G2 pool is cut uniformly.  zk_groth16_shard_range is that rule (pure host arithmetic, heavy_prefix = 0
 * for the uniform cut); zk_groth16_pool_layout reports the slices a key actually holds. */
#define ZK_GROTH16_PARTIAL_BYTES 768
int zk_groth16_shard_range(uint64_t points, uint64_t heavy_prefix, uint32_t rank, uint32_t world, uint64_t* lo, uint64_t* hi);
int zk_groth16_pk_upload_sharded(uint32_t n, uint32_t m, const zk_csr* L, const zk_csr* R, const zk_csr* O,
                                 const uint8_t* mid, const uint8_t* pk_g1, size_t pk_g1_points,
                                 const uint8_t* pk_g2, size_t pk_g2_points, uint32_t rank, uint32_t world,
                                 uint64_t* handle);
int zk_groth16_prove_partial(uint64_t handle, const uint8_t* sol, const uint8_t r[32], const uint8_t s[32],
                             uint8_t partial[ZK_GROTH16_PARTIAL_BYTES]);
/* pipelined form (slots as in zk_groth16_prove_async): the exchange and combine of one proof run on
 * the host while the GPU is already working on the partial sums of the next ones */
int zk_groth16_prove_partial_async(uint64_t handle, const uint8_t* sol, const uint8_t r[32], const uint8_t s[32], uint32_t slot);
int zk_groth16_prove_partial_wait(uint64_t handle, uint32_t slot, uint8_t partial[ZK_GROTH16_PARTIAL_BYTES]);
/* Distributed Fr stage (the form bench.py uses at N > 1).  Proofs are handled in groups of N: rank j runs the
 * Fr stage of the j-th proof of the group ONCE (instead of every rank running it for every proof) and leaves the
 * three scalar vectors over the FULL pools (p1, p1 and p2 canonical Fr elements, see zk_groth16_pool_layout) in
 * caller-owned device buffers; the host framework exchanges the slices (one all-to-all over RCCL / xGMI: rank g
 * receives [lo_g, hi_g) of every proof of the group); zk_groth16_msm_partial_async then runs the three MSMs of
 * one proof over this rank's slice from such a device buffer, and zk_groth16_prove_partial_wait returns its
 * 768-byte partial sums for the all-gather + zk_groth16_combine as above.  Replaces the same reference code
 * (groth16.ml:123-161); QAP.eval (QAP.ml:120-135) is the first half, the apply_powers folds the second.
 * The device pointers are plain HBM addresses (hipMalloc / a framework tensor's data pointer). */
int zk_groth16_pool_layout(uint64_t handle, uint64_t* p1, uint64_t* p2, uint64_t* lo1, uint64_t* hi1, uint64_t* lo2, uint64_t* hi2);
int zk_groth16_scalars_async(uint64_t handle, const uint8_t* sol, const uint8_t r[32], const uint8_t s[32], uint32_t slot,
                             void* d_scal_a /* p1 * 32 B */, void* d_scal_c /* p1 * 32 B */, void* d_scal_b /* p2 * 32 B */);
int zk_groth16_scalars_wait(uint64_t handle, uint32_t slot);    /* ZK_ERR_REMAINDER / ZK_ERR_SCALAR_RANGE as zk_groth16_prove */
int zk_groth16_msm_partial_async(uint64_t handle, uint32_t slot, const void* d_scal_a_slice /* (hi1-lo1) * 32 B */,
                                 const void* d_scal_c_slice, const void* d_scal_b_slice /* (hi2-lo2) * 32 B */);
/* plain device memory for callers without a framework allocator */
int zk_device_malloc(size_t bytes, void** dptr);
int zk_device_free(void* dptr);
int zk_device_memcpy(void* dst, const void* src, size_t bytes);   /* any direction, synchronous */
int zk_groth16_combine(const uint8_t* partials /* world * 768 */, uint32_t world, uint8_t proof[384]);
/* Device-resident form of the exchange (the path RCCL takes: slot buffer -> all-gather on a DEVICE tensor -> combine, no PCIe hop in between):
 * _wait_device waits like zk_groth16_prove_partial_wait and leaves the 768-byte block at the DEVICE address d_partial (same return codes);
 * _combine_device reads `world` blocks from DEVICE memory, block j at d_partials + j * stride_bytes (stride >= 768: the all-gather of a whole
 * round of proofs lands as [rank][proof][768]), adds them on the GPU and returns the proof.  Same group elements, same bytes
 * (groth16.ml:123-161: the proof does not depend on how the sums were cut). */
int zk_groth16_prove_partial_wait_device(uint64_t handle, uint32_t slot, void* d_partial /* device, 768 B */);
int zk_groth16_combine_device(const void* d_partials /* device */, size_t stride_bytes, uint32_t world, uint8_t proof[384]);

/* ---- protocol seam: Pinocchio.Make(C).{NonZK,ZK}.prove (src/pinocchio/pinocchio.ml:536-538,559-561) ----
 * Evaluation key of pinocchio.ml:37-60 flattened per group (maps in Var.Map key order over I_mid, resp.
 * over all m variables for v_all / w_all; lists as stored):
 *   g1: vv | yy | vav | yay | bvwy  (n_mid each) | si (n+1) | v_all (m) | w_all (m) | vt | yt | vavt | yayt | vbt | wbt | ybt
 *   g2: ww | waw (n_mid each) | si2 (n+1, not used by the prover) | wt | wawt
 * zk_pinocchio_prove = ZKCompute.f (:427-514) with dv, dw, dy supplied in the order the reference draws
 * them (:428-430); all three zero gives Compute.f (:210-248), i.e. NonZK.prove.
 * Precondition: si[0] is the G1 generator (ZK_ERR_ARG otherwise).  ZKCompute.f subtracts `one * dy` with G1.one (:485), not a point of the key, and
 * the library lets that term ride on si[0]; every key KeyGen.generate makes has si[0] = [s^0] = one.  No other relation between key points is assumed.
 * proof: vv (G1) | ww (G2) | yy | h | vavv | waww (G2) | yayy | bvwy = 960 B uncompressed, the field order
 * of Compute.proof (:195-208).  ZK_ERR_REMAINDER as for Groth16.
 * The h product's points v_all | w_all carry the blinding terms sum_k (dw c_k) [v_k(s)] + sum_k (dv c_k) [w_k(s)] (:481-486) = dw [v(s)] + dv [w(s)]
 * with v = sum_k c_k v_k, w = sum_k c_k w_k -- the polynomials QAP.eval builds anyway.  At upload the library checks v_all / w_all against the
 * key's own powers (<v_all, rho> = <si, coefficients of sum_k rho_k v_k> for a pseudo-random rho, likewise w_all: true of every key
 * KeyGen.generate makes, :104-109,140-147; rho is seeded from a digest of the uploaded si | v_all | w_all bytes and from entropy drawn once per process,
 * so it cannot be known when a key is written -- the check promises the compact pool only to keys that satisfy the relation, up to the 2^-64 of the
 * seed; it does not validate a key in any other respect) and then lets the two terms ride on si: the COMPACT h pool, n + 1 points instead of n + 1 + 2 m, same
 * proof bytes.  A key that fails the check, or any key under zk_set_option("ZK_PIN_COMPACT_H", "0"), keeps the full pool and is used point by
 * point as ZKCompute.f uses it.  Products that carry the SAME scalar vector -- vv|vt and vav|vavt, yy|yt and yay|yayt, ww|wt and waw|wawt (:438-447,
 * 489-498) -- share one counting sort of it when their base sets have the same identity pattern (true of generated keys; decided per key at upload;
 * "ZK_PIN_SHARED_SORT" = "0" switches it off). */
int zk_pinocchio_pk_upload(uint32_t n, uint32_t m, const zk_csr* L, const zk_csr* R, const zk_csr* O,
                           const uint8_t* mid, const uint8_t* pk_g1, size_t pk_g1_points,
                           const uint8_t* pk_g2, size_t pk_g2_points, uint64_t* handle);
/* As zk_groth16_pk_derive_lagrange, for the evaluation key of pinocchio.ml:37-60: the powers si are turned into the Lagrange basis of the points
 * n .. 2n-2 in the exponent (plus [Z(s)] = <si, Z>, once), so that h enters its multi-scalar product through VALUES; v(s), w(s) never needed
 * coefficient vectors (they come from the per-variable pools).  Once per key; proofs byte-identical.  With the compact h pool the blinding terms
 * follow: v = kappa_v X^(n-1) + (degree <= n-2), so dw [v(s)] + dv [w(s)] ride on [lambda_t(s)] through the values v(n+t), w(n+t) the prover
 * already extrapolates, plus ONE more base [s^(n-1)] = si[n-1] for the leading coefficients. */
int zk_pinocchio_pk_derive_lagrange(uint64_t handle);
/* zk_pinocchio_pk_upload plus the n points h_lagrange = [lambda_t(s)] (n-1) | [Z(s)] (lambda_t the Lagrange basis of the points n .. 2n-2): the first n
 * points of pool 5 after zk_pinocchio_pk_derive_lagrange, for a host that knows s or stored a derived key.  Runs the ordinary upload (every check,
 * the one behind the compact h pool included), decodes and checks h_lagrange like any key point (encoding, curve, [r] P = O unless
 * ZK_KEY_SUBGROUP_CHECK=0), and installs pool 5 exactly as the derivation does: h_lagrange | si[0] | si[n-1], or h_lagrange | si[0] | v_all | w_all for a
 * full pool.  That h_lagrange belongs to the key's si is the CALLER'S PROMISE, as for zk_groth16_pk_upload_lagrange: the library does not check it, and
 * points that break it give proofs that do not verify.  Device lists of one entry only (ZK_ERR_ARG otherwise). */
int zk_pinocchio_pk_upload_lagrange(uint32_t n, uint32_t m, const zk_csr* L, const zk_csr* R, const zk_csr* O, const uint8_t* mid,
                                    const uint8_t* pk_g1, size_t pk_g1_points, const uint8_t* pk_g2, size_t pk_g2_points,
                                    const uint8_t* h_lagrange /* n * 96 */, uint64_t* handle);
/* KeyGen.generate, pinocchio.ml:77-189, in one call; arguments, forms, handle and status codes as zk_groth16_keygen (no trapdoor value is refused
 * but one >= r: the reference divides by none -- each of rv, rw, s, av, aw, ay, b, gm may be 0, and s may be a point of the domain 0 .. n-1
 * (t = Z(s) = 0: vt .. ybt, wt, wawt and the verification key's yt are the identity) or of n .. 2n-2; the key is the reference's, sound or not).
 *   toxic = rv | rw | s | av | aw | ay | b | gm (:83-91);  pk_g1 / pk_g2: the layouts of zk_pinocchio_pk_upload, 5 |mids| + (n+1) + 2m + 7 and
 *   2 |mids| + (n+1) + 2 points;  vk_g1 = one | aw | bgm | vv_io | yy_io (3 + 2 n_io), vk_g2 = one2 | av | ay | gm2 | bgm2 | yt | ww_io (6 + n_io), :62-75.
 *   The handle's h pool is compact whenever ZK_PIN_COMPACT_H allows it: a generated key satisfies the relation behind it by construction, so the
 *   check of the upload is not run; ZK_PIN_SHARED_SORT is decided as at upload.  ZK_KEY_FORM_LAGRANGE: pool 5 as after zk_pinocchio_pk_derive_lagrange. */
int zk_pinocchio_keygen(uint32_t n, uint32_t m, const zk_csr* L, const zk_csr* R, const zk_csr* O, const uint8_t* mid,
                        const uint8_t toxic[256], uint32_t form,
                        uint8_t* pk_g1, size_t pk_g1_points, uint8_t* pk_g2, size_t pk_g2_points,
                        uint8_t* vk_g1 /* (3 + 2 n_io) * 96 */, uint8_t* vk_g2 /* (6 + n_io) * 192 */, uint64_t* handle);
/* A resident base pool of the key as uncompressed points, in pool order (out == NULL: only *count).  Pools 0..5 are the G1 products
 * vv|vt, yy|yt, vav|vavt, yay|yayt, bvwy|vbt|wbt|ybt and the h pool; 6..7 the G2 products ww|wt and waw|wawt (pinocchio.ml:37-60).
 * The h pool by key form:  compact (default): si (n + 1 points); after zk_pinocchio_pk_derive_lagrange [lambda_t(s)] (n-1) | [Z(s)] | [1] | [s^(n-1)];
 *                          full:              si | v_all | w_all;   after the derivation [lambda_t(s)] | [Z(s)] | [1] | v_all | w_all. */
int zk_pinocchio_pool_points(uint64_t handle, int pool, uint8_t* out, size_t capacity_points, size_t* count);
/* The wire forms ("keys and base lists in WIRE form" above; pinocchio.ml:37-60 through curve.ml:199-219) */
int zk_pinocchio_pk_upload_compressed(uint32_t n, uint32_t m, const zk_csr* L, const zk_csr* R, const zk_csr* O, const uint8_t* mid,
                                      const uint8_t* pk_g1 /* points * 48 */, size_t pk_g1_points, const uint8_t* pk_g2 /* points * 96 */, size_t pk_g2_points,
                                      const uint8_t* h_lagrange /* n * 48, or NULL */, uint64_t* handle);
int zk_pinocchio_pool_points_compressed(uint64_t handle, int pool, uint8_t* out, size_t capacity_points, size_t* count);
int zk_pinocchio_pk_free(uint64_t handle);
int zk_pinocchio_prove(uint64_t handle, const uint8_t* sol, const uint8_t dv[32], const uint8_t dw[32],
                       const uint8_t dy[32], uint8_t proof[960]);
/* Pipelined form, as for Groth16: up to 15 proofs in flight on one key, each on its own `slot`;
 * sol == NULL uses the witness made resident by zk_pinocchio_set_witness.  zk_pinocchio_prove == _async + _wait on slot 0. */
int zk_pinocchio_reserve_slots(uint64_t handle, uint32_t count);
int zk_pinocchio_set_witness(uint64_t handle, const uint8_t* sol);
int zk_pinocchio_prove_async(uint64_t handle, const uint8_t* sol, const uint8_t dv[32], const uint8_t dw[32],
                             const uint8_t dy[32], uint32_t slot);
int zk_pinocchio_prove_wait(uint64_t handle, uint32_t slot, uint8_t proof[960]);

/* ---- a batch of witnesses in one call, the proofs out as WIRE bytes ------------------------------------------------------------------------
 * Groth16.prove (groth16.ml:123-161,235-237) and ZKCompute.f / Compute.f (pinocchio.ml:427-514) over `count` witnesses on one key, every proof
 * written as the reference's proof record holds it (groth16.ml:110-114, pinocchio.ml:195-208: compressed points, 48 B per G1 and 96 B per G2 point in
 * declaration order) -- the bytes zk_*_verify_resident_compressed take and the strings of the record's JSON.  The call keeps `in_flight` proofs in
 * flight on slots 0 .. in_flight-1 of the handle (allocated as zk_*_reserve_slots allocates them), each in the form that leaves its sums on the
 * device, collects them in one slab (at most 8192 proofs each) and converts a whole slab at once: one lane per point, one inversion, the sign bit,
 * one copy to the host.  Per proof the host waits for one event; there is no conversion launch and no copy per proof.
 *   sols: witness i at sols + i * m * 32, or NULL: the witness made resident by zk_*_set_witness, for every proof.
 *   rs / blind: the randomness of proof i in the order the reference draws it (groth16.ml:124-125: r | s; pinocchio.ml:428-430: dv | dw | dy; all
 *     zero gives Compute.f, NonZK.prove).
 *   in_flight: 1 .. 15; 0 = the library's default, 14 (what the headline rate is measured with); never more than count.  Every slot holds the working
 *     memory of a proof: a caller short of device memory passes a smaller number.
 *   proofs: proof i at proofs + i * 192 (A 48 | B 96 | C 48) or + i * 480 (vv 48 | ww 96 | yy 48 | h 48 | vavv 48 | waww 96 | yayy 48 | bvwy 48),
 *     byte for byte what zk_g1/g2_compress give for the points zk_groth16_prove / zk_pinocchio_prove returns for the same handle, witness and
 *     randomness; the identity is C0 00 .. 00.
 *   status[i]: the code that single call would return -- ZK_OK, ZK_ERR_REMAINDER, ZK_ERR_SCALAR_RANGE.  The bytes of a failed proof are ALL ZERO:
 *     no compression flag, so no verifier takes them for a proof (zk_*_verify_resident_compressed: ZK_ERR_ARG).  A failed proof changes nothing for
 *     its neighbours.  The call returns ZK_OK when the batch ran, whatever the statuses.
 * Before the device is touched: null rs / blind, proofs or status, in_flight > 15, count > 2^24 -> ZK_ERR_ARG; count = 0 -> ZK_OK, nothing is touched;
 * an unknown handle -> ZK_ERR_HANDLE (without a GPU: ZK_ERR_HIP); null sols without a resident witness -> ZK_ERR_ARG; a proof in flight on any slot
 * of the handle -> ZK_ERR_ARG, and that proof stays collectable.  Afterwards every slot is idle and the single calls give the bytes they gave before.
 * Every key form of a one-device handle is served (tau powers, Lagrange uploaded, derived, generated, uploaded compressed).  A handle over a device
 * list of several entries is served with the same bytes, proof by proof through the per-proof path with ONE proof in flight (in_flight is not read),
 * then the same conversion on the first device.  The shards of the one-process-per-GPU path (zk_groth16_pk_upload_sharded, zk_groth16_pk_shard)
 * produce partial sums only: ZK_ERR_ARG.  Kernel k_proofs_to_wire (profiles/prove_many_kernel_resources.txt), timer family prove_to_wire. */
int zk_groth16_prove_many_compressed(uint64_t handle,
        const uint8_t* sols   /* count * m * 32, or NULL: the resident witness for every proof */,
        const uint8_t* rs     /* count * 64: r | s of proof i, the order the reference draws them */,
        uint32_t count, uint32_t in_flight /* 1..15; 0 = library default */,
        uint8_t* proofs       /* count * 192: A 48 | B 96 | C 48 */,
        int32_t* status       /* count */);
int zk_pinocchio_prove_many_compressed(uint64_t handle,
        const uint8_t* sols, const uint8_t* blind /* count * 96: dv | dw | dy */,
        uint32_t count, uint32_t in_flight,
        uint8_t* proofs       /* count * 480: vv | ww | yy | h | vavv | waww | yayy | bvwy */,
        int32_t* status);

/* ---- verify surface (scope row f1): Curve.S.Pairing.pairing (src/lib/zk/curve.mli:46-54) ---------------
 * Host code (a handful of pairings per proof, as in the reference, where they are calls into its external
 * library): Groth16 verify = 3 pairings (groth16.ml:163-173), Pinocchio Verify.f = 13 (pinocchio.ml:254-420).
 * zk_pairing_product: gt_out = prod_i e(P_i, Q_i) with one final exponentiation; points uncompressed as
 * everywhere else, checked for curve and subgroup membership.  GT encoding: the 12 Fp coefficients of the tower
 * Fp12 = Fp6[w]/(w^2 - v), Fp6 = Fp2[v]/(v^3 - (1+u)) in the order c0.c0.a, c0.c0.b, c0.c1.a, ..., c1.c2.b,
 * 48 B big-endian each (the reference's GT bytes are defined by its external library: parity unpinned there,
 * compared as field elements here).  zk_pairing_check: *is_one = (product == 1). */
int zk_pairing_product(const uint8_t* g1_points, const uint8_t* g2_points, size_t n, uint8_t gt_out[576]);
int zk_pairing_check(const uint8_t* g1_points, const uint8_t* g2_points, size_t n, int* is_one);
/* Groth16.verify (groth16.ml:163-173): *ok = [ e(A,B) == ab * e(sum_k io_k * ltgm_io_k, gm) * e(C, d) ];
 * ab = e(alpha, beta) in the GT encoding above, io_scalars the public coefficients in the key's variable order. */
int zk_groth16_verify(const uint8_t ab[576], const uint8_t* ltgm_io /* n_io * 96 */, const uint8_t* io_scalars /* n_io * 32 */,
                      size_t n_io, const uint8_t gm[192], const uint8_t d[192], const uint8_t proof[384], int* ok);
/* Pinocchio Verify.f (pinocchio.ml:254-420), verification key (pinocchio.ml:62-75) flattened:
 *   vk_g1 = one | aw | bgm | vv_io[n_io] | yy_io[n_io]      vk_g2 = one2 | av | ay | gm2 | bgm2 | yt | ww_io[n_io] */
int zk_pinocchio_verify(const uint8_t* vk_g1, const uint8_t* vk_g2, const uint8_t* io_scalars, size_t n_io,
                        const uint8_t proof[960], int* ok);

/* ---- the same three on the device, many per call (zukelang_amd/csrc/pairing_dev.hip: the products; zukelang_amd/csrc/verify_resident.hip: the verifiers)
 * The calls above cost one host core milliseconds to tens of milliseconds each; a host that checks a stream of proofs hands them over in batches instead.  All three run on
 * the first device of the list, are synchronous, keep nothing after they return, check their arguments before they touch the device and return
 * ZK_ERR_HIP where there is none: the device path has no CPU fallback.  A lone proof is quicker through the host calls (profiles/verify_many.json).
 * zk_pairing_product_many (Pairing.pairing, curve.mli:46-54): `count` products; product k takes lens[k] pairs, the pairs of all products
 * concatenated in g1_points / g2_points.  gt_out block k = the 576 bytes zk_pairing_product returns for those pairs (lens[k] = 0, or an identity on
 * either side of every pair: 1).  Every point is checked as there (encoding, curve, subgroup); a bad point fails the whole call with the code of the
 * FIRST bad point in the host's decoding order (G1 of pair i, then G2 of pair i), and gt_out then holds nothing to rely on. */
int zk_pairing_product_many(const uint8_t* g1_points, const uint8_t* g2_points, const uint64_t* lens, uint32_t count,
                            uint8_t* gt_out /* count * 576 */);
/* Groth16.verify (groth16.ml:163-173) of `count` proofs under one key, the key laid out as for zk_groth16_verify.  A null argument or a bad key
 * point fails the call with that function's code.  A proof's own defects never do: ok[i] = its *ok, status[i] = the code the single-proof call
 * would return for proof i under this key -- ZK_OK; ZK_ERR_ARG / ZK_ERR_NOT_ON_CURVE for the first bad point of the proof in the order A, B, C;
 * ZK_ERR_SCALAR_RANGE for a public input >= r -- and ok[i] = 0 whenever status[i] != 0.  status may be NULL.  count = 0: ZK_OK, nothing touched.
 * A malformed ab compares unequal to every product, as on the host: every ok[i] = 0.
 *   What runs is the pipeline of the resident keys below, on a key that lives for this call: the key's points are decoded and checked, its IO points
 *   become narrow window tables (one per 8192 points: n_io has no limit), and per slab of proofs one H2D copy (proofs | public inputs), every proof
 *   point decoded and checked once, the statuses, one short product per proof and table, the three pairs per proof assembled on the device, Miller
 *   loops, final exponentiations, the comparison with ab, and one D2H copy (ok | status).  The key's points and the first slab's proof points are
 *   checked side by side, on two streams of the device.  The key is in no handle table and is gone, with its workspaces, when the call returns:
 *   the call keeps nothing.  The subgroup test of every point is [r] P = O.  Kernel families under
 *   zk_profile_get: pairing_point_checks, msm_short, pairing_miller, pairing_final_exp. */
int zk_groth16_verify_many(const uint8_t ab[576], const uint8_t* ltgm_io, size_t n_io, const uint8_t gm[192], const uint8_t d[192],
                           const uint8_t* io_scalars /* count * n_io * 32 */, const uint8_t* proofs /* count * 384 */, uint32_t count,
                           uint8_t* ok /* count */, int32_t* status /* count, may be NULL */);
/* Pinocchio Verify.f (pinocchio.ml:254-420) of `count` proofs under one key, vk_g1 / vk_g2 as for zk_pinocchio_verify; ok and status as above, the
 * points of a proof in the order vv, ww, yy, h, vavv, waww, yayy, bvwy.  The same pipeline on a key that lives for the call: three short products per
 * proof and table (vv_io, yy_io in G1, ww_io in G2), vio + vv, yio + yy and wio + ww added on the device, thirteen pairs in five products per proof,
 * each compared with 1.  The same kernel families. */
int zk_pinocchio_verify_many(const uint8_t* vk_g1, const uint8_t* vk_g2, size_t n_io,
                             const uint8_t* io_scalars /* count * n_io * 32 */, const uint8_t* proofs /* count * 960 */, uint32_t count,
                             uint8_t* ok /* count */, int32_t* status /* count, may be NULL */);

/* ---- verification keys resident on the device (zukelang_amd/csrc/verify_resident.hip) ----------------------
 * A verifier checks a stream of proofs under ONE key (Groth16.verify, groth16.ml:163-173; Verify.f, pinocchio.ml:254-420), and the key's points pass
 * of_bytes_exn once when the key is read (curve.ml:199-212), not once per proof.  The _many calls above build the key, and allocate its workspaces,
 * in every call; a handle does it once, at upload, and keeps on the device: gm and d (Pinocchio: the nine fixed key points) as decoded points, the IO points as a
 * narrow window table for one short product per proof, the 576 bytes of ab as given, and workspaces that grow on demand and are reused.  A verify
 * call then costs one H2D copy (proofs | public inputs), the kernels and one D2H copy (ok | status).
 *   Upload: the key laid out as for zk_groth16_verify / zk_pinocchio_verify.  Every point is checked (encoding: ZK_ERR_ARG; curve and subgroup:
 *   ZK_ERR_NOT_ON_CURVE); a bad point fails the upload with the code, and in the order, the _many call reports it (Groth16: gm, d, ltgm_io[k]), and
 *   no handle is made.  The subgroup test is by endomorphism -- P in G1 <=> [z^2] P = (beta^2 x, -y), Q in G2 <=> psi(Q) = [z] Q: 2 x 63 and 63
 *   doublings instead of the 254 of [r] P = O -- the same predicate on every point of the curve.  A malformed ab is kept: every ok is then 0, as
 *   above.  n_io = 0 is legal; n_io > 8192 -> ZK_ERR_ARG (the table of the short products; the _many calls have no such limit).
 *   Verify: ok and status are byte for byte those of zk_groth16_verify_many / zk_pinocchio_verify_many on the same key and inputs.  An unknown or
 *   freed handle, or a handle of the other protocol -> ZK_ERR_HANDLE; then count = 0 -> ZK_OK, nothing touched; a null pointer (status excepted;
 *   io_scalars when n_io = 0) -> ZK_ERR_ARG; count > 2^24 -> ZK_ERR_ARG.  Without a GPU every upload is ZK_ERR_HIP, so no handle exists.
 *   The handle lives on the first device of the list at upload, is called from one host thread like the key handles, and counts as a live key
 *   handle for zk_set_devices / zk_set_device_list; zk_shutdown frees it.  Kernel families under zk_profile_get: verify_point_checks, msm_short,
 *   pairing_miller, pairing_final_exp.  No option is read. */
int zk_groth16_vk_upload(const uint8_t ab[576], const uint8_t* ltgm_io /* n_io * 96 */, size_t n_io, const uint8_t gm[192], const uint8_t d[192],
                         uint64_t* handle);
int zk_pinocchio_vk_upload(const uint8_t* vk_g1, const uint8_t* vk_g2, size_t n_io, uint64_t* handle);
int zk_vk_info(uint64_t handle, int* protocol /* 0 Groth16, 1 Pinocchio */, uint64_t* n_io);   /* any out may be NULL */
int zk_vk_free(uint64_t handle);
int zk_groth16_verify_resident(uint64_t handle, const uint8_t* io_scalars /* count * n_io * 32 */, const uint8_t* proofs /* count * 384 */,
                               uint32_t count, uint8_t* ok /* count */, int32_t* status /* count, may be NULL */);
int zk_pinocchio_verify_resident(uint64_t handle, const uint8_t* io_scalars /* count * n_io * 32 */, const uint8_t* proofs /* count * 960 */,
                                 uint32_t count, uint8_t* ok /* count */, int32_t* status /* count, may be NULL */);
/* One answer for a whole batch under a resident Groth16 key: are ALL of these proofs good?  Instead of one pairing equation per proof (Groth16.verify,
 * groth16.ml:163-173, as the reference's harness loops over it, test.ml:107-179) the equations are raised to coefficients rho_i and multiplied:
 *     prod_i e([rho_i] A_i, B_i) . e(-sum_k t_k ltgm_io_k, gm) . e(-sum_i [rho_i] C_i, d) = ab^S,   t_k = sum_i rho_i w_ik (mod r),  S = sum_i rho_i
 * -- per batch one final exponentiation, one product over the public inputs and two Miller loops; per proof one Miller loop, two 128-bit multiples in
 * G1 and n_io multiply-adds in Fr.  status[i] is byte for byte what zk_groth16_verify_resident reports for proof i (the same decoder, subgroup and
 * range tests, the same order); a proof with a non-zero status does not enter the fold (identity pairs, no rho).  *all_ok = 1 if and only if every
 * status is 0 and the folded equation holds.  The per-proof call stays the way to learn WHICH proof is bad once this one has said that one is.
 *   THE CONTRACT FOR rho.  The caller draws every rho_i (16 bytes, little-endian like the ABI's scalars, non-zero) from a cryptographic generator
 *   AFTER the proofs are fixed, and keeps them unpredictable to whoever made the proofs.  A batch that holds a bad proof then passes with probability
 *   at most 2^-128.  With rho known or chosen in advance a bad batch CAN pass: two proofs whose C are shifted by +D and -D cancel under equal
 *   coefficients (tests/test_gpu_verify_folded.py shows it).  The library draws nothing itself: it has no generator to vouch for.
 *   vk_handle: from zk_groth16_vk_upload.  Refused before the device is touched, with ZK_ERR_ARG: all_ok, proofs or rho null (count > 0), a zero
 *   rho_i, count > 2^24.  Then a Pinocchio, freed or unknown handle -> ZK_ERR_HANDLE (a non-zero handle without a usable GPU: ZK_ERR_HIP, no handle
 *   can exist); count = 0 -> ZK_OK, *all_ok = 1, nothing else touched; io_scalars null with n_io > 0 -> ZK_ERR_ARG.  More than 8192 proofs are
 *   folded slab by slab into state kept on the device; the equation is decided once.  Kernel families: verify_point_checks, verify_fold_scale,
 *   pairing_miller, verify_fold_tree, msm_short, pairing_final_exp, verify_fold_pow. */
int zk_groth16_verify_folded(uint64_t vk_handle, const uint8_t* io_scalars /* count * n_io * 32 */, const uint8_t* proofs /* count * 384 */,
                             const uint8_t* rho /* count * 16 */, uint32_t count, int* all_ok, int32_t* status /* count, may be NULL */);
/* The same one answer under a resident Pinocchio key.  Verify.f (pinocchio.ml:254-420) decides five equations per proof -- the vv check (285), the ww
 * check (298), the yy check (311), the bvwy check (361-366) and divisibility (418-420).  Equation e of proof i is raised to a coefficient rho_ie, all
 * of them are multiplied, and the pairs are collected by their fixed key point:
 *     prod_i e([rho_i4](vio_i + vv_i), wio_i + ww_i)
 *       . e(S_av, av) e(-(S_one2 + S_yio), one2) e(S_ay, ay) e(S_gm2, gm2) e(-S_bgm2, bgm2) e(-S_yt, yt) . e(aw, T_aw) e(-one, T_one) e(-bgm, T_bgm) = 1
 *     S_av = sum_i [rho_i0] vv_i     S_one2 = sum_i ([rho_i0] vavv_i + [rho_i2] yayy_i + [rho_i4] yy_i)     S_ay = sum_i [rho_i2] yy_i
 *     S_gm2 = sum_i [rho_i3] bvwy_i  S_bgm2 = sum_i [rho_i3](vv_i + yy_i)   S_yt = sum_i [rho_i4] h_i    S_yio = sum_k t_k yy_io_k, t_k = sum_i rho_i4 w_ik
 *     T_aw = sum_i [rho_i1] ww_i     T_one = sum_i [rho_i1] waww_i          T_bgm = sum_i [rho_i3] ww_i   (G2)
 * with vio_i, wio_i the sums over the public inputs as the per-proof call forms them.  Per proof one Miller loop and two short products instead of
 * thirteen Miller loops, five final exponentiations and three short products; per batch nine Miller loops and one final exponentiation, and no power
 * in GT: the right-hand side is 1.  status[i] is byte for byte what zk_pinocchio_verify_resident reports for proof i; a proof with a non-zero status
 * enters nothing (no pair, no summand, no share of t).  *all_ok = 1 if and only if every status is 0 and the folded equation holds.
 *   THE CONTRACT FOR rho.  FIVE coefficients per proof, rho_i0 .. rho_i4, one per equation in the order above, 16 bytes each, little-endian, every
 *   one non-zero.  The caller draws all of them from a cryptographic generator AFTER the proofs are fixed, and keeps them unpredictable to whoever
 *   made the proofs.  A batch that holds a bad proof then passes with probability at most 2^-128.  With coefficients known or chosen in advance a bad
 *   batch CAN pass, in two ways (tests/test_gpu_pinocchio_verify_folded.py shows both): ACROSS proofs -- vavv of two proofs moved by +D and -D cancels
 *   when rho_00 = rho_10 -- and INSIDE one proof -- vavv moved by +D and yayy by -D both meet one2 and cancel when rho_i0 = rho_i2.  The second way is
 *   why a proof has five independent coefficients and not one: with one, a single proof could trade an error of one equation against another's.
 *   vk_handle: from zk_pinocchio_vk_upload.  Refused before the device is touched, with ZK_ERR_ARG: all_ok, proofs or rho null (count > 0), a zero
 *   among the 5 count coefficients, count > 2^24.  Then a Groth16, freed or unknown handle -> ZK_ERR_HANDLE (a non-zero handle without a usable GPU:
 *   ZK_ERR_HIP); count = 0 -> ZK_OK, *all_ok = 1, nothing else touched; io_scalars null with n_io > 0 -> ZK_ERR_ARG.  More than 8192 proofs are
 *   folded slab by slab into state kept on the device; the equation is decided once.  Kernel families: verify_point_checks, msm_short,
 *   verify_fold_scale (the G1 multiples, every sum, the scalars), verify_fold_scale_g2 (the G2 multiples), pairing_miller, verify_fold_tree,
 *   pairing_final_exp.  Measured on an MI355X against zk_pinocchio_verify_resident: faster at 4096 and 16384 proofs, slower at 256 and
 *   below. */
int zk_pinocchio_verify_folded(uint64_t vk_handle, const uint8_t* io_scalars /* count * n_io * 32 */, const uint8_t* proofs /* count * 960 */,
                               const uint8_t* rho /* count * 80: rho_i0 .. rho_i4, 16 B little-endian each */, uint32_t count,
                               int* all_ok, int32_t* status /* count, may be NULL */);

/* ---- the same four calls on proofs in their COMPRESSED wire form (zukelang_amd/csrc/verify_resident.hip) ----------------------
 * The reference's proof is a record of compressed points (groth16.ml:110-114, pinocchio.ml:195-208; to_compressed_bytes, curve.ml:199-219): 48 B per
 * G1 point, 96 B per G2 point, in declaration order -- Groth16 A 48 | B 96 | C 48 = 192 B; Pinocchio vv 48 | ww 96 | yy 48 | h 48 | vavv 48 | waww 96 |
 * yayy 48 | bvwy 48 = 480 B.  These calls take the proofs as they arrive and decompress them on the device, in the same call: one H2D copy of
 * proofs | public inputs (| rho) at the compressed stride, one decompression launch per group straight out of that buffer -- one lane per point, the
 * square root by ONE power (p - 3) / 4 in Fp and TWO in Fp2, no inversion -- then the handle's subgroup test, by endomorphism, and from there the
 * very code of the uncompressed call.  Signatures, argument checks and their order, handle checks, count = 0, count > 2^24, the no-GPU case
 * (ZK_ERR_HIP) and the slabs of 8192 proofs are those of the twin without _compressed; everything the twin refuses before the device is touched is
 * refused here before the device is touched.
 *   status[i] is the code zk_g1_decompress / zk_g2_decompress returns for the FIRST bad point of proof i, in the order a verifier meets them (A, B, C;
 *   vv, ww, yy, h, vavv, waww, yayy, bvwy): ZK_ERR_ARG for a bad encoding (the compression bit missing, a coordinate >= p, the infinity bit on
 *   anything but C0 00 .. 00), ZK_ERR_NOT_ON_CURVE for an abscissa that is on no point of the curve or a point outside the subgroup; otherwise
 *   ZK_ERR_SCALAR_RANGE for a public input >= r; otherwise 0.  For a proof whose points all decode, ok[i] and status[i] are byte for byte what the
 *   uncompressed call returns on the same handle for the decompressed proof, and *all_ok follows the same rule.  The folded calls keep THE CONTRACT
 *   FOR rho above, unchanged.  Kernel families: verify_point_decompress (the decompression launches), then the twin's (the subgroup test stays under
 *   verify_point_checks).
 *   zk_groth16_verify_many / zk_pinocchio_verify_many, whose key lives for one call, have no compressed form: a caller with proofs off the wire
 *   checks a stream of them under one key and has every reason to hold a handle. */
int zk_groth16_verify_resident_compressed(uint64_t handle, const uint8_t* io_scalars /* count * n_io * 32 */,
                                          const uint8_t* proofs /* count * 192: A 48 | B 96 | C 48 */, uint32_t count, uint8_t* ok /* count */,
                                          int32_t* status /* count, may be NULL */);
int zk_pinocchio_verify_resident_compressed(uint64_t handle, const uint8_t* io_scalars /* count * n_io * 32 */,
                                            const uint8_t* proofs /* count * 480: vv 48 | ww 96 | yy 48 | h 48 | vavv 48 | waww 96 | yayy 48 | bvwy 48 */,
                                            uint32_t count, uint8_t* ok /* count */, int32_t* status /* count, may be NULL */);
int zk_groth16_verify_folded_compressed(uint64_t vk_handle, const uint8_t* io_scalars /* count * n_io * 32 */, const uint8_t* proofs /* count * 192 */,
                                        const uint8_t* rho /* count * 16 */, uint32_t count, int* all_ok, int32_t* status /* count, may be NULL */);
int zk_pinocchio_verify_folded_compressed(uint64_t vk_handle, const uint8_t* io_scalars /* count * n_io * 32 */, const uint8_t* proofs /* count * 480 */,
                                          const uint8_t* rho /* count * 80 */, uint32_t count, int* all_ok, int32_t* status /* count, may be NULL */);

/* ---- measurement hooks (bench.py) ----------------------------------------------------------------
 * With profiling on, kernel families are bracketed by HIP events on the stream they run on;
 * zk_profile_get returns the summed milliseconds and launch count since the last reset. */
int zk_profile_enable(int level);   /* 0 off | 1 the MSM accumulate kernels only (cheap: safe inside a timed region) | 2 every family */
int zk_profile_reset(void);
int zk_profile_get(const char* family, double* total_ms, uint64_t* launches);
int zk_profile_names(char* buf, size_t buflen);   /* comma-separated family names */
/* Work counters gathered at level 2 (one proof at a time) since the last reset, e.g. "msm_accumulate_g1:entries" (sorted (point, window) entries),
 * ":copies" (first entries of a chunk or run: no field product), ":second_steps" (6-product additions of two affine points), ":full_additions". */
int zk_profile_counter(const char* name, uint64_t* value);
int zk_sync(void);                                 /* waits for everything the library has enqueued on every device of its list, the per-slot
                                                      streams of proofs in flight included (hipDeviceSynchronize per device) */
/* Throughput of the register-resident Montgomery multiplier (kind 0 = Fr, 1 = Fp): ALU ceiling.
 * kind | 4: one wave on the whole chip (dependent-chain latency).  kind | 8: the best rate over 2 / 4 / 6 / 8 waves per SIMD. */
int zk_bench_field_mul(int kind, uint32_t iters, double* gmul_per_s);
/* Field-layer self-test hook (tests/test_gpu_field.py): for each of n (even) operand pairs a_i, b_i < p (48-byte little-endian
 * integers) the device evaluates 23 base-field expressions through the lazy-reduction code paths of the group law and
 * returns them fully reduced (23 x 48 B per pair, little-endian); pairs (2k, 2k+1) also act as one Fp2 operand pair. */
int zk_selftest_fp(const uint8_t* a, const uint8_t* b, size_t n, uint8_t* out);
/* The scalar field on 8 x 32-bit words (tests/test_gpu_fr_field.py): the Fe<FrParams> functions of csrc/ff.cuh -- the arithmetic of the sparse products,
 * the R1CS check, the factorial tables, the keygen scans and every to/from-Montgomery pass -- one lane per element.  a, b: 32-byte little-endian integers.
 * op 0: a_i, b_i < r (anything else -> ZK_ERR_ARG), taken into Montgomery form on the device; out: 14 x 32 B per pair, little-endian, canonical, out of
 *   Montgomery form:   0 a + b   1 a - b   2 b - a   3 a b   4 a^2   5 -a   6 2a (fe_dbl)   7 1 / a (0 for 0)   8 fe_from_mont(fe_to_mont(a))
 *   9 fe_from_u32 of a's low word   10 a b + a a + b b, accumulated term by term as a row of zk_fr_spmv is   11 flags: bit 0 fe_is_zero(a), bit 1 fe_eq(a, b)
 *   12 a through the 9 x 29-bit form and back, fr9_canon_pack(fr9_unpack(a R))   13 a b as the NTT kernels multiply, fr9_mul(unpack(a R), unpack(32 b R)),
 *   with the factor convention of csrc/fr29.cuh, packed canonically.
 * op 1: any 256-bit a_i; b is not read and may be NULL; out: 1 byte per element, fe_is_canonical(a_i) = (a_i < r).
 * A null pointer, n = 0, another op -> ZK_ERR_ARG before the device is touched. */
int zk_selftest_fr(int op, const uint8_t* a, const uint8_t* b, size_t n, uint8_t* out);
/* The scalar field of the NTT kernels on bare limbs (tests/test_gpu_fr_field.py): the fr9_* functions of csrc/fr29.cuh on lazily reduced integers of
 * 9 limbs of 29 bits, so the caller chooses the representation and can put a butterfly at the bounds of the stage schedule (csrc/ntt_lds.cuh), which no
 * input of zk_fr_ntt does.  operands: n x 3 values u, v, w of 9 words each (27 words per lane).  u, and v where the op reads it, are weakly normalised:
 * limbs 0..7 at most 2^29 + 7, top limb at most that of 64 r, (64 r) >> 232.  w, where the op reads it, is a factor as memory holds one: limbs 0..7 at
 * most 2^29 - 1 and a value below r.  Keeping the VALUE bounds of each function (csrc/fr29.cuh) is the caller's part.  out: raw limbs, not reduced further:
 *   op 0  fr9_canon_pack(u), 8 words          op 1  fr9_reduce_weak(u), 9 words          op 2  fr9_mul(u, v), 9 words
 *   op 3  the forward butterfly in the order of lds_ntt_stages<false>, 5 x 9 words: x = fr9_add(u, v) | fr9_reduce_weak(x) | fr9_mul(fr9_sub_raw<5>(u, v), w) |
 *         fr9_mul(fr9_sub<5>(u, v), w) | fr9_sub<5>(u, v) (the span-2 stage)
 *   op 4  the inverse butterfly, 3 x 9 words: t = fr9_mul(v, w) | fr9_add(u, t) | fr9_sub<2>(u, t)
 *   op 5  fr9_pack_exact(fr9_unpack(x)), 8 words, x = the first 8 words of u taken as ANY 256-bit value (no limb rule applies).
 * A null pointer, n = 0, another op, a limb or a top limb out of range, a w with inexact limbs or a value >= r -> ZK_ERR_ARG before the device is touched. */
int zk_selftest_fr29(int op, const uint32_t* operands, size_t n, uint32_t* out);
/* The paired field products (tests/test_gpu_fp_paired.py): two or three independent products of the group law run side by side where the products are
 * expanded in place.  operands: n x 4 values a, b, c, d as their 14 limbs of 29 bits in a 16-word slot each (64 words per lane), weakly normalised --
 * every limb at most 2^29 + 7, top limb at most 64 * 13 (every value below the at-rest bound 64 p qualifies) -- so the caller chooses the representation.
 * out: 13 x 48 B per lane, little-endian, fully reduced, each the Montgomery product x y / 2^406 mod p:
 *   0, 1  a b | c d      2, 3  a^2 | c^2      4, 5  a b | a b      6, 7  a b | c a      8, 9  a b | c d with each output written over an input
 *   10, 11, 12  a b - c d | a d | c b (the fused double product with its lazily negated factor beside two plain products).
 * A null pointer, n = 0, a limb or a top limb out of range -> ZK_ERR_ARG before the device is touched. */
int zk_selftest_fp_paired(const uint32_t* operands, size_t n, uint8_t* out);
/* Two Fp2 products on a lane pair, one whole lazy-Karatsuba product per lane (tests/test_gpu_fp2_lanewise.py): what the G2 bucket accumulation issues.
 * operands: n x 4 values a, b, c, d of Fp2, each as c0 | c1, each component as its 14 limbs of 29 bits in a 16-word slot (128 words per quadruple),
 * weakly normalised as for zk_selftest_fp_paired.  out: 3 x 96 B per quadruple (c0 | c1, 48 B each, little-endian, fully reduced), each a Montgomery
 * product x y / 2^406 in Fp2:   0  a b      1  c d      2  a b - c d (the fused end of a mixed addition).
 * A null pointer, n = 0, a limb or a top limb out of range -> ZK_ERR_ARG before the device is touched. */
int zk_selftest_fp2_lanewise(const uint32_t* operands, size_t n, uint8_t* out);
/* The base field under its products, on bare limbs (tests/test_gpu_fp29.py): the additive forms of csrc/ff.cuh with their tables of spread multiples of p,
 * the full reduction, the zero test, the dense memory format and the lockstep inversion of csrc/fp_inv.cuh.  operands: n x 3 values a, b, c as their 14 limbs
 * of 29 bits in a 16-word slot each (48 words per lane); slots an op does not read are not looked at.  Unless stated otherwise an operand is weakly
 * normalised -- limbs 0..12 at most 2^29 + 7 -- and its top limb is at most that of its value bound B, (B p) >> 377; keeping the VALUE below B p is the
 * caller's part.  out: raw limbs (14 words) with no reduction beyond what the function under test does, unless stated otherwise.
 *   op 0   fp_canon_call(a), a < 8192 p: the exact limbs of a mod p
 *   op 1   fp_carry(a): a is ANY 14 words (no limb rule; the top limb is taken modulo 2^32)
 *   op 2   fe_add(a, b), a, b < 64 p          op 3   fe_dbl(a), a < 64 p
 *   op 4   the first 12 words of a are a dense 384-bit value below p (anything else -> ZK_ERR_ARG): fp_unpack of it (14 words) | fp_pack of that (12 words)
 *   op 5   a in EXACT limbs (at most 2^29 - 1) and below p (anything else -> ZK_ERR_ARG), taken as the plain integer X: fp_inv29_call(X) as it returns it,
 *          weakly normalised limbs of X^-1 mod p with a value in (4 p, 60 p), 0 for 0 (14 words) | fe_inv_fast of the same limbs, fully reduced: X^-1 2^812 mod p (14 words)
 *   op 8, 9, 10   fe_is_zero<B>(a), a < B p, B = 2, 64 (the at-rest bound), 192 (the largest any call site instantiates).  One flag word: bit 0 as a unit
 *          without ZK_FP_INLINE_MUL compiles it (slow path fp_canon), bit 1 as a unit with it does (slow path fp_is_zero_mod_p_inline), bit 2
 *          fp_is_zero_mod_p_inline(a) called directly (a = k p for k = limb0 / p mod 2^29)
 *   op 16 + k, k = 0..11    fe_sub<64, B>(a, b): a - b + 2^(k+1) p through row k of FP29_KP; a < 64 p, b < B p, B = 1 for k = 0 and 2^k otherwise
 *   op 32 + k, k = 0..12    fe_neg<B>(a): 2^(k+1) p - a through row k of FP29_KP; a < B p, B as above
 *   op 48 + k, k = 0..12    fe_neg_lazy<B>(a): the same through row k of FP29_KPN with NO carry pass: limbs in [1, 2^30]
 *   op 64 + k, k = 1..11    fe_sub_sub_dbl<64, B, B>(a, b, c): a - b - 2 c + 2^(k+1) p through row k of FP29_KPW; a < 64 p, b, c < B p, B = 1 for k = 1 and 2^(k-1) otherwise
 * These are all the rows a function can be instantiated with under FP_MAX_BOUND = 8192.
 * A null pointer, n = 0, n >= 2^24, another op, a limb or a top limb out of range, an operand that is not canonical where the op needs one -> ZK_ERR_ARG
 * before the device is touched. */
int zk_selftest_fp29(int op, const uint32_t* operands, size_t n, uint32_t* out);
/* Square roots as the decompression kernels take them (tests/test_gpu_field.py): n elements of Fp (field 0: 48 B big-endian each) or Fp2 (field 1:
 * 96 B each, imaginary part | real part, the order of a G2 coordinate on the wire), one lane per element.  is_square[i] = 1 / 0; root[i] = of the two
 * roots the one the ZCash sign rule calls the larger (Fp2: by the imaginary part, by the real part when that is zero) -- decided by the same device
 * function as the sign bit of zk_g1/g2_decompress_batch -- and zeros when there is none.  An element >= p -> ZK_ERR_ARG. */
int zk_selftest_sqrt(int field, const uint8_t* a, size_t n, uint8_t* root, uint8_t* is_square);
/* The device's Fp12 (tests/test_gpu_pairing.py): n elements in the GT encoding through the functions the pairing kernels call, one group of lanes
 * per element.  op 0: a b | 1: a^2 | 2: 1 / a (0 for 0) | 3: conjugate a^(p^6) | 4: Frobenius a^p | 5: a^(p^2) | 6: a times the sparse element made
 * of b's coefficients of w^0, w^3, w^5 (the shape of a Miller line: c0.c0, c1.c1, c1.c2) | 7: a^((p^12 - 1) / r).  b is read by ops 0 and 6.
 * A coefficient >= p -> ZK_ERR_ARG. */
int zk_selftest_fp12(int op, const uint8_t* a, const uint8_t* b, size_t n, uint8_t* out);
/* The two subgroup kernels side by side (tests/test_gpu_subgroup_endo.py): n uncompressed points of group 0 (G1, 96 B) or 1 (G2, 192 B) through the
 * decoder and then method 0: [r] P = O (what the _many verifiers and the key uploads run) | 1: by endomorphism (what the resident verification keys
 * run).  verdict[i] = 0 good (the identity included) | 2 bad encoding | 1 not on the curve | 4 on the curve, outside the subgroup.  A null pointer,
 * n = 0, another group or method -> ZK_ERR_ARG before the device is touched. */
int zk_selftest_subgroup(int group, int method, const uint8_t* points, size_t n, uint8_t* verdict);
/* The front half of a compressed slab on bare points (tests/test_gpu_point_decompress.py): n compressed points of group 0 (G1, 48 B) or 1 (G2, 96 B)
 * through the very kernels the *_compressed verifiers launch -- the decompression, then the subgroup test by endomorphism.  verdict[i] = 0 good (the
 * identity included) | 2 bad encoding | 1 the abscissa is on no point of the curve | 4 on the curve, outside the subgroup.  out[i] = the decoded point
 * in the ABI's uncompressed bytes (96 / 192 B) when the verdict is 0 or 4, zero bytes otherwise.  A null pointer, n = 0 or another group -> ZK_ERR_ARG
 * before the device is touched. */
int zk_selftest_point_decompress(int group, const uint8_t* in /* n * 48 | n * 96 */, size_t n, uint8_t* out /* n * 96 | n * 192 */, uint8_t* verdict);
/* The conversion launch of zk_*_prove_many_compressed on points the caller chooses (tests/test_gpu_prove_many.py): n pairs of an affine point of group
 * 0 (G1, 96 B) or 1 (G2, 192 B) in the ABI's uncompressed bytes and a scalar 0 < z < r (32 B little-endian).  The device forms the XYZZ point
 * (x z^2, y z^3, z^2, z^3) -- the all-zero pair stands for the identity (zz = 0) -- and runs k_proofs_to_wire on the n points as a batch of n proofs
 * of one point each; out[i] = the point's wire bytes, what zk_g1/g2_compress give for (x, y).  Neither curve nor subgroup is checked: a test can feed
 * coordinates no proof reaches.  A null pointer, n = 0, n >= 2^24 or another group -> ZK_ERR_ARG before the device is touched; a coordinate >= p, z = 0
 * or z >= r -> ZK_ERR_ARG. */
int zk_selftest_proof_wire(int group, const uint8_t* affine /* n * 96 | 192 */, const uint8_t* z /* n * 32, 0 < z < r */, size_t n,
                           uint8_t* out /* n * 48 | 96 */);
/* Every form of the device's group law on bare operands (tests/test_gpu_group_law.py), each run by a kernel of the translation unit that builds the
 * form for production, with that unit's flags.  group 0 = G1, 1 = G2 (on lane pairs).  a[i]: an XYZZ point as four field elements x, y, zz, zzz
 * (x_affine = x / zz, y_affine = y / zzz, zz^3 = zzz^2; zz = 0 is the identity whatever x and y are), each 48 B big-endian -- in G2 96 B, imaginary
 * part | real part -- so the caller chooses the representation.  b[i] by form: a second XYZZ point | an affine point x, y (all zeros = the identity,
 * where the form accepts it) | ignored (may be null) | a canonical scalar of 32 B, little-endian.  out[i]: the result, uncompressed, the identity as
 * the library encodes it.
 *   form  0 xyzz_add_impl          b XYZZ      4 xyzz_madd_impl, identity q allowed  b affine     11 xyzz_add_slots   b XYZZ
 *         1 xyzz_dbl_impl          -           5 xyzz_madd_impl, table entries       b affine     12 xyzz_dbl_slots   -
 *         2 xyzz_dbl_aff (a has                (never the identity)                               13 jac_dbl          -
 *           zz = zzz = 1, or is                6 xyzz_mmadd_impl (a has zz = zzz = 1 b affine     14 jac_madd         b affine, never the identity
 *           the identity)          -             or is the identity)                              15 jac_add          b XYZZ
 *         3 xyzz_add_raw_mem       b XYZZ      7, 8, 9 = 4, 5, 6 with the field products expanded in place        16 xyzz_mul_scalar_endo  b scalar
 *                                              10 xyzz_madd_parked (G2 only), table entries       b affine
 * rep 0: the coordinates enter the form canonical.  rep 1: the kernel first lifts every operand to x + k p, the largest k its type in the form's
 * production caller admits (csrc/group_selftest.cuh lists them), so that the form's zero tests see multiples of p.
 * A null pointer, n = 0, an unknown group / form / rep, a coordinate >= p, an identity b where the form excludes it -> ZK_ERR_ARG; a scalar >= r ->
 * ZK_ERR_SCALAR_RANGE; all before the device is touched. */
int zk_selftest_group(int group, int form, int rep, const uint8_t* a, const uint8_t* b, size_t n, uint8_t* out);
/* The tail of zk_groth16_pk_contribute on a caller's list (tests/test_gpu_contribute.py): out[i] = k pts[i] for n uncompressed G1 points (the identity as
 * the library encodes it, or all zeros; it stays the identity) and ONE canonical scalar k of 32 B, little-endian (0 is served: every product is the
 * identity).  slab: points per chain of launches, 0 = the call's default of 2^18, so that a list of a few hundred points can cross a slab boundary.  A
 * null pointer, n = 0 or k >= r -> ZK_ERR_ARG before the device is touched; a coordinate >= p -> ZK_ERR_ARG, a point off the curve -> ZK_ERR_NOT_ON_CURVE. */
int zk_selftest_g1_scale(const uint8_t* pts /* n * 96 */, size_t n, const uint8_t k[32], uint32_t slab /* 0 = default */, uint8_t* out /* n * 96 */);
/* The column sums of zk_groth16_pk_specialize on a caller's list (tests/test_gpu_colsum.py): out[k] = sum over e in [col_ptr[k], col_ptr[k+1]) of
 * coef[e] * pts[row[e]] for n_pts uncompressed G1 points (the identity as the library encodes it, or all zeros) and m columns, through the call's own
 * stages: the split of the entries by coefficient class, the compacted multiplications, the chunked sums and their levels.  An empty column gives the
 * identity; a row may repeat within a column.  A null pointer, n_pts = 0, m = 0, a col_ptr that is not monotone, a row >= n_pts -> ZK_ERR_ARG, a
 * coefficient >= r -> ZK_ERR_SCALAR_RANGE, all before the device is touched; a coordinate >= p -> ZK_ERR_ARG, a point off the curve -> ZK_ERR_NOT_ON_CURVE. */
int zk_selftest_g1_colsum(const uint8_t* pts /* n_pts * 96 */, size_t n_pts, const uint32_t* col_ptr /* m + 1 */, const uint32_t* row /* nnz */,
                          const uint8_t* coef /* nnz * 32 */, uint32_t m, uint8_t* out /* m * 96 */);
/* zk_groth16_verify_folded stopped before the comparison (tests/test_gpu_verify_folded.py): both sides of the folded equation as GT encodings --
 * lhs_gt the final exponentiation of the product of the count + 2 Miller values, rhs_gt = ab^S -- and the two sums that enter the key's pairs,
 * sum_c = sum_i [rho_i] C_i and sum_io = sum_k t_k ltgm_io_k, un-negated, uncompressed (the identity as the library encodes it).  Same arguments and
 * refusals as the call itself; count = 0 or a null output -> ZK_ERR_ARG. */
int zk_selftest_groth16_fold(uint64_t vk_handle, const uint8_t* io_scalars, const uint8_t* proofs, const uint8_t* rho, uint32_t count,
                             uint8_t lhs_gt[576], uint8_t rhs_gt[576], uint8_t sum_c[96], uint8_t sum_io[96], int32_t* status);
/* zk_pinocchio_verify_folded stopped before the comparison (tests/test_gpu_pinocchio_verify_folded.py): lhs_gt = the final exponentiation of the
 * product of all count + 9 Miller values, and the ten sums that enter the key's pairs, un-negated, uncompressed (the identity as the library encodes
 * it): sums_g1 = S_av | S_one2 (the proofs' part only, without S_yio) | S_ay | S_gm2 | S_bgm2 | S_yt | S_yio, sums_g2 = T_aw | T_one | T_bgm.  Same
 * arguments and refusals as the call itself; count = 0 or a null output -> ZK_ERR_ARG. */
int zk_selftest_pinocchio_fold(uint64_t vk_handle, const uint8_t* io_scalars, const uint8_t* proofs, const uint8_t* rho, uint32_t count,
                               uint8_t lhs_gt[576], uint8_t sums_g1[7 * 96], uint8_t sums_g2[3 * 192], int32_t* status);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif

#ifdef __cplusplus
}
#endif
#endif
