(* mi355x.ml -- ctypes binding of libzkmi355x (include/zkmi355x.h), the MI355X prove path.

   Goes to src/lib/zk/ of the zukelang tree (library `zk`, plus `ctypes ctypes.foreign` in its dune stanza: see ocaml/dune).
   Every entry point an OCaml host needs is bound here; the header says which reference interface each one replaces.
   This file cannot be compiled in the image it was written in (no OCaml toolchain there); tests/test_ocaml_binding.py
   holds every symbol name and every arity below against the header and the built library.

   Conventions of the C side: Fr = 32 B little-endian (Bls12_381.Fr.to_bytes), G1 / G2 = 96 / 192 B uncompressed
   (G1.to_bytes / G2.to_bytes), all buffers caller-owned, 0 = ok, negative = error code. *)

open Ctypes
open Foreign

let lib =
  let file = try Sys.getenv "ZK_LIBZKMI355X_PATH" with Not_found -> "libzkmi355x.so" in
  Dl.dlopen ~filename:file ~flags:[ Dl.RTLD_NOW ]

let fn name typ = foreign ~from:lib name typ

(* ------------------------------------------------------------------ small helpers *)

let u32 = Unsigned.UInt32.of_int
let u64 = Unsigned.UInt64.of_int
let sz = Unsigned.Size_t.of_int
let bytes_start = ocaml_bytes_start
let cat = Bytes.concat Bytes.empty
let null_bytes : char ptr = from_voidp char null

(* an OCaml buffer copied into C memory, for the few arguments that live in a C struct *)
let carray_of_bytes (b : bytes) : char CArray.t =
  let a = CArray.make char (max 1 (Bytes.length b)) in
  Bytes.iteri (fun i c -> CArray.set a i c) b;
  a

(* ------------------------------------------------------------------ errors
   The reference raises exceptions; the C side returns codes (header, "Errors").
     ZK_ERR_APPLY_POWERS (-6)  -> Invalid_argument "apply_powers"        curve.ml:116
     ZK_ERR_REMAINDER (-4)     -> Assert_failure (QAP.ml:134: assert (Polynomial.is_zero rem))
     ZK_ERR_DOMAIN (-8)        -> Assert_failure (curve.ml:96-100: assert false in G.dot)
     ZK_ERR_NOT_ON_CURVE (-2)  -> Bls12_381.G1.Not_on_curve              what of_bytes_exn raises on such bytes (curve.ml:199-212)
     ZK_ERR_SCALAR_RANGE (-3)  -> Bls12_381.Fr.Not_in_field              what Fr.of_bytes_exn raises on a value >= r
     anything else             -> Failure with the library's text
   Not_on_curve / Not_in_field are the exception constructors of opam bls12-381 6.1.0 (its source is not vendored in zukelang;
   if a later version renames them this is the one place to touch). *)

let zk_strerror = fn "zk_strerror" (int @-> returning string)
let zk_last_error = fn "zk_last_error" (void @-> returning string)

let check rc =
  if rc = 0 then ()
  else
    let detail () = zk_strerror rc ^ ": " ^ zk_last_error () in
    match rc with
    | -6 -> invalid_arg "apply_powers"
    | -4 -> raise (Assert_failure ("QAP.ml", 134, 4))
    | -8 -> raise (Assert_failure ("curve.ml", 100, 8))
    | -2 -> raise (Bls12_381.G1.Not_on_curve (Bytes.of_string (detail ())))
    | -3 -> raise (Bls12_381.Fr.Not_in_field (Bytes.of_string (detail ())))
    | _ -> failwith (detail ())

(* ------------------------------------------------------------------ devices and options *)

let zk_device_count = fn "zk_device_count" (void @-> returning int)
let zk_init = fn "zk_init" (int @-> returning int)
let zk_shutdown = fn "zk_shutdown" (void @-> returning int)
let zk_set_devices = fn "zk_set_devices" (uint64_t @-> returning int)
let zk_sync = fn "zk_sync" (void @-> returning int)
let zk_get_device_list = fn "zk_get_device_list" (ptr int32_t @-> uint32_t @-> ptr uint32_t @-> returning int)

(* entries of the library's device list (0 before the first call that binds a device): more than one after zk_set_devices / use_all_devices *)
let device_list_length () =
  let n = allocate uint32_t Unsigned.UInt32.zero in
  check (zk_get_device_list (from_voidp int32_t null) (u32 0) n);
  Unsigned.UInt32.to_int !@n

(* knobs that are not test-only, by name (the environment stays a fallback): see the header *)
let zk_set_option = fn "zk_set_option" (string @-> string @-> returning int)

(* all MI355X of the node behind every key uploaded afterwards (header, "multi-device keys") *)
let use_all_devices () =
  let n = zk_device_count () in
  if n > 1 then check (zk_set_devices (Unsigned.UInt64.of_int ((1 lsl n) - 1)))

(* ------------------------------------------------------------------ Fr stage: FFT.ml:69-105 *)

let zk_fr_ntt = fn "zk_fr_ntt" (ocaml_bytes @-> uint32_t @-> int @-> returning int)

let zk_fr_poly_mul =
  fn "zk_fr_poly_mul" (ocaml_bytes @-> size_t @-> ocaml_bytes @-> size_t @-> ocaml_bytes @-> ptr size_t @-> returning int)

(* ------------------------------------------------------------------ curve plugin seam: curve.ml:94-118,180 *)

let zk_msm_g1 =
  fn "zk_msm_g1" (ocaml_bytes @-> size_t @-> ocaml_bytes @-> size_t @-> uint32_t @-> ocaml_bytes @-> returning int)

let zk_msm_g2 =
  fn "zk_msm_g2" (ocaml_bytes @-> size_t @-> ocaml_bytes @-> size_t @-> uint32_t @-> ocaml_bytes @-> returning int)

let zk_g1_of_fr = fn "zk_g1_of_fr" (ocaml_bytes @-> size_t @-> ocaml_bytes @-> returning int)
let zk_g2_of_fr = fn "zk_g2_of_fr" (ocaml_bytes @-> size_t @-> ocaml_bytes @-> returning int)
let zk_g1_powers = fn "zk_g1_powers" (uint32_t @-> ocaml_bytes @-> ocaml_bytes @-> returning int)
let zk_g2_powers = fn "zk_g2_powers" (uint32_t @-> ocaml_bytes @-> ocaml_bytes @-> returning int)

(* sum_i scalars_i * points_i over byte strings; 96 or 192 bytes per point *)
let msm ~g2 (points : bytes) (scalars : bytes) : bytes =
  let psize = if g2 then 192 else 96 in
  let out = Bytes.create psize in
  let f = if g2 then zk_msm_g2 else zk_msm_g1 in
  check
    (f (bytes_start points) (sz (Bytes.length points / psize)) (bytes_start scalars) (sz (Bytes.length scalars / 32)) (u32 0)
       (bytes_start out));
  out

(* resident MSM bases (header, "resident MSM bases"): a point list uploaded and checked once, then multiplied many times.  The errors map as
   for msm: Invalid_argument "apply_powers" when a product is longer than the list (curve.ml:116). *)
let zk_bases_upload = fn "zk_bases_upload" (int @-> ocaml_bytes @-> size_t @-> ptr uint64_t @-> returning int)
let zk_bases_info = fn "zk_bases_info" (uint64_t @-> ptr int @-> ptr uint64_t @-> ptr uint64_t @-> returning int)
let zk_bases_free = fn "zk_bases_free" (uint64_t @-> returning int)
let zk_msm_resident = fn "zk_msm_resident" (uint64_t @-> ocaml_bytes @-> size_t @-> ocaml_bytes @-> returning int)

let zk_msm_resident_many =
  fn "zk_msm_resident_many" (uint64_t @-> ocaml_bytes @-> ptr uint64_t @-> uint32_t @-> ocaml_bytes @-> returning int)

let resident_upload ~g2 (points : bytes) : Unsigned.UInt64.t =
  let psize = if g2 then 192 else 96 in
  let h = allocate uint64_t Unsigned.UInt64.zero in
  check (zk_bases_upload (if g2 then 1 else 0) (bytes_start points) (sz (Bytes.length points / psize)) h);
  !@h

let resident_free (h : Unsigned.UInt64.t) = ignore (zk_bases_free h)

(* [g * s_0; g * s_1; ...] for the group's generator g: G.of_Fr mapped over a list (curve.ml:180), one kernel launch *)
let of_fr_many ~g2 (scalars : bytes) : bytes =
  let psize = if g2 then 192 else 96 in
  let n = Bytes.length scalars / 32 in
  let out = Bytes.create (max 1 (psize * n)) in
  if n > 0 then check ((if g2 then zk_g2_of_fr else zk_g1_of_fr) (bytes_start scalars) (sz n) (bytes_start out));
  Bytes.sub out 0 (psize * n)

(* of_compressed_bytes_exn over a whole list on the GPU (a key read from the reference's JSON: every point is compressed there): the compressed points
   back to back in, the uncompressed points back to back out; Not_on_curve / Invalid_argument as the one-point functions of Bls12_381 raise *)
let zk_g1_decompress_batch = fn "zk_g1_decompress_batch" (ocaml_bytes @-> size_t @-> ocaml_bytes @-> returning int)
let zk_g2_decompress_batch = fn "zk_g2_decompress_batch" (ocaml_bytes @-> size_t @-> ocaml_bytes @-> returning int)

let decompress_many ~g2 (comp : bytes) : bytes =
  let csize = if g2 then 96 else 48 in
  let n = Bytes.length comp / csize in
  if Bytes.length comp <> n * csize then invalid_arg "decompress_many";
  let out = Bytes.create (max 1 (2 * csize * n)) in
  if n > 0 then check ((if g2 then zk_g2_decompress_batch else zk_g1_decompress_batch) (bytes_start comp) (sz n) (bytes_start out));
  Bytes.sub out 0 (2 * csize * n)

let powers ~g2 d (s : bytes) : bytes =
  let psize = if g2 then 192 else 96 in
  let out = Bytes.create (psize * (d + 1)) in
  check ((if g2 then zk_g2_powers else zk_g1_powers) (u32 d) (bytes_start s) (bytes_start out));
  out

(* ------------------------------------------------------------------ circuits: three CSR matrices (header, zk_csr) *)

type csr
let csr : csr structure typ = structure "zk_csr"
let csr_row_ptr = field csr "row_ptr" (ptr uint32_t)
let csr_col = field csr "col" (ptr uint32_t)
let csr_val = field csr "val" (ptr char)
let () = seal csr

(* One matrix, built from rows of (column, 32-byte coefficient) in ascending column order; the record keeps the C arrays alive. *)
type matrix = { c : csr structure; keep_ptr : Unsigned.uint32 CArray.t; keep_col : Unsigned.uint32 CArray.t; keep_val : char CArray.t }

let matrix_of_rows (rows : (int * bytes) list list) : matrix =
  let nnz = List.fold_left (fun a r -> a + List.length r) 0 rows in
  let keep_ptr = CArray.make uint32_t (List.length rows + 1) in
  let keep_col = CArray.make uint32_t (max 1 nnz) in
  let keep_val = CArray.make char (max 1 (32 * nnz)) in
  CArray.set keep_ptr 0 (u32 0);
  let e = ref 0 in
  List.iteri
    (fun g row ->
      List.iter
        (fun (k, coeff) ->
          CArray.set keep_col !e (u32 k);
          Bytes.iteri (fun i ch -> CArray.set keep_val ((32 * !e) + i) ch) coeff;
          incr e)
        row;
      CArray.set keep_ptr (g + 1) (u32 !e))
    rows;
  let c = make csr in
  setf c csr_row_ptr (CArray.start keep_ptr);
  setf c csr_col (CArray.start keep_col);
  setf c csr_val (CArray.start keep_val);
  { c; keep_ptr; keep_col; keep_val }

(* y = M x over Fr for one sparse matrix (header: zk_fr_spmv): QAP.eval's sums at the gates' points, or -- M transposed, x = the Lagrange basis at
   tau -- every u_k(tau) of a keygen at once, where the reference runs Poly.apply per variable *)
let zk_fr_spmv = fn "zk_fr_spmv" (uint32_t @-> uint32_t @-> ptr csr @-> ocaml_bytes @-> ocaml_bytes @-> returning int)

(* l_i(x), i < n, over the QAP's points first .. first+n-1 and Z(x) (header: zk_fr_lagrange_at): what Poly.apply gives for the n interpolation
   polynomials and the target (QAP.ml:84-100), exact for every x, the domain's own points included *)
let zk_fr_lagrange_at = fn "zk_fr_lagrange_at" (uint32_t @-> uint32_t @-> ocaml_bytes @-> ocaml_bytes @-> ocaml_bytes @-> returning int)

let lagrange_at ~n ~first (x : bytes) : bytes * bytes =
  let out = Bytes.create (32 * n) and z = Bytes.create 32 in
  check (zk_fr_lagrange_at (u32 n) (u32 first) (bytes_start x) (bytes_start out) (bytes_start z));
  (out, z)

(* ------------------------------------------------------------------ key generation in one call (header: zk_groth16_keygen, zk_pinocchio_keygen)
   groth16.ml:45-108 and pinocchio.ml:77-189: the trapdoor goes in (canonical Fr bytes, in the order Fr.gen is called), the key's bytes in the
   reference's format come out together with a live handle -- ZK_KEY_FORM_LAGRANGE: the handle already holds the Lagrange form, the fast prover's. *)

let key_form_tau_powers = 0
let key_form_lagrange = 1

let zk_groth16_keygen =
  fn "zk_groth16_keygen"
    (uint32_t @-> uint32_t @-> ptr csr @-> ptr csr @-> ptr csr @-> ocaml_bytes @-> ocaml_bytes @-> uint32_t @-> ocaml_bytes @-> size_t
   @-> ocaml_bytes @-> size_t @-> ocaml_bytes @-> ocaml_bytes @-> ptr uint64_t @-> returning int)

let zk_pinocchio_keygen =
  fn "zk_pinocchio_keygen"
    (uint32_t @-> uint32_t @-> ptr csr @-> ptr csr @-> ptr csr @-> ocaml_bytes @-> ocaml_bytes @-> uint32_t @-> ocaml_bytes @-> size_t
   @-> ocaml_bytes @-> size_t @-> ocaml_bytes @-> ocaml_bytes @-> ptr uint64_t @-> returning int)

(* one keygen call: (pk_g1, pk_g2, vk_g1, vk_g2, handle option); the *_points are the lengths the header gives for this circuit.  A handle can only
   be had on a device list of ONE entry (header); on a longer list -- after use_all_devices -- the call is made with handle = NULL (the bytes can
   be had on any list) and returns None: the caller then uploads the bytes, which builds the multi-device key behind one handle as before. *)
let keygen_call f ~n ~m (l : matrix) (r : matrix) (o : matrix) ~(mid : bytes) ~(toxic : bytes) ~form ~g1_points ~g2_points ~vk1_points ~vk2_points =
  let g1 = Bytes.create (96 * g1_points) and g2 = Bytes.create (192 * g2_points) in
  let vk1 = Bytes.create (96 * vk1_points) and vk2 = Bytes.create (192 * vk2_points) in
  let want_handle = device_list_length () <= 1 in
  let h = allocate uint64_t Unsigned.UInt64.zero in
  check
    (f (u32 n) (u32 m) (addr l.c) (addr r.c) (addr o.c) (bytes_start mid) (bytes_start toxic) (u32 form) (bytes_start g1) (sz g1_points)
       (bytes_start g2) (sz g2_points) (bytes_start vk1) (bytes_start vk2)
       (if want_handle then h else from_voidp uint64_t null));
  (g1, g2, vk1, vk2, if want_handle then Some !@h else None)

(* ------------------------------------------------------------------ a phase-1 string specialised to a circuit (header: zk_groth16_pk_specialize)
   srs_g1 = tau1[max(n+2, 2n-1)] | alpha_tau1[n] | beta_tau1[n], srs_g2 = beta2 | tau2[n+2], uncompressed: the key of the trapdoor
   (alpha, beta, 1, 1, tau) comes out, bytes and handle as from keygen_call, and no secret went in.  The string is trusted: check the key. *)

let zk_groth16_srs_sizes = fn "zk_groth16_srs_sizes" (uint32_t @-> ptr uint64_t @-> ptr uint64_t @-> ptr uint64_t @-> returning int)

let zk_groth16_pk_specialize =
  fn "zk_groth16_pk_specialize"
    (uint32_t @-> uint32_t @-> ptr csr @-> ptr csr @-> ptr csr @-> ocaml_bytes @-> ocaml_bytes @-> size_t @-> ocaml_bytes @-> size_t @-> uint32_t
   @-> ocaml_bytes @-> size_t @-> ocaml_bytes @-> size_t @-> ocaml_bytes @-> ocaml_bytes @-> ptr uint64_t @-> returning int)

(* the call's column sums on a caller's list (the library's own tests): pts, n_pts, col_ptr, row, coef, m, out *)
let zk_selftest_g1_colsum =
  fn "zk_selftest_g1_colsum" (ocaml_bytes @-> size_t @-> ptr uint32_t @-> ptr uint32_t @-> ocaml_bytes @-> uint32_t @-> ocaml_bytes @-> returning int)

(* (points of tau1, of alpha_tau1 and beta_tau1 each, of tau2) for n constraints *)
let groth16_srs_sizes ~n : int * int * int =
  let a = allocate uint64_t Unsigned.UInt64.zero and b = allocate uint64_t Unsigned.UInt64.zero and c = allocate uint64_t Unsigned.UInt64.zero in
  check (zk_groth16_srs_sizes (u32 n) a b c);
  (Unsigned.UInt64.to_int !@a, Unsigned.UInt64.to_int !@b, Unsigned.UInt64.to_int !@c)

(* one specialisation: (pk_g1, pk_g2, vk_g1, vk_g2, handle option), the handle under the rule of keygen_call *)
let specialize_call ~n ~m (l : matrix) (r : matrix) (o : matrix) ~(mid : bytes) ~(srs_g1 : bytes) ~(srs_g2 : bytes) ~form ~g1_points ~g2_points ~vk1_points
    ~vk2_points =
  let g1 = Bytes.create (96 * g1_points) and g2 = Bytes.create (192 * g2_points) in
  let vk1 = Bytes.create (96 * vk1_points) and vk2 = Bytes.create (192 * vk2_points) in
  let want_handle = device_list_length () <= 1 in
  let h = allocate uint64_t Unsigned.UInt64.zero in
  check
    (zk_groth16_pk_specialize (u32 n) (u32 m) (addr l.c) (addr r.c) (addr o.c) (bytes_start mid) (bytes_start srs_g1)
       (sz (Bytes.length srs_g1 / 96))
       (bytes_start srs_g2)
       (sz (Bytes.length srs_g2 / 192))
       (u32 form) (bytes_start g1) (sz g1_points) (bytes_start g2) (sz g2_points) (bytes_start vk1) (bytes_start vk2)
       (if want_handle then h else from_voidp uint64_t null));
  (g1, g2, vk1, vk2, if want_handle then Some !@h else None)

(* ------------------------------------------------------------------ Groth16: groth16.ml:24-34,116-161,235-237 *)

let zk_groth16_pk_upload =
  fn "zk_groth16_pk_upload"
    (uint32_t @-> uint32_t @-> ptr csr @-> ptr csr @-> ptr csr @-> ocaml_bytes @-> ocaml_bytes @-> size_t @-> ocaml_bytes @-> size_t
   @-> ptr uint64_t @-> returning int)

let zk_groth16_pk_derive_lagrange = fn "zk_groth16_pk_derive_lagrange" (uint64_t @-> returning int)
let zk_groth16_pk_free = fn "zk_groth16_pk_free" (uint64_t @-> returning int)

let zk_groth16_prove =
  fn "zk_groth16_prove" (uint64_t @-> ocaml_bytes @-> ocaml_bytes @-> ocaml_bytes @-> ocaml_bytes @-> returning int)

(* the same entry point taking the witness made resident by zk_groth16_set_witness (sol = NULL) *)
let zk_groth16_prove_resident =
  fn "zk_groth16_prove" (uint64_t @-> ptr char @-> ocaml_bytes @-> ocaml_bytes @-> ocaml_bytes @-> returning int)

let zk_groth16_reserve_slots = fn "zk_groth16_reserve_slots" (uint64_t @-> uint32_t @-> returning int)
let zk_groth16_set_witness = fn "zk_groth16_set_witness" (uint64_t @-> ocaml_bytes @-> returning int)

let zk_groth16_prove_async =
  fn "zk_groth16_prove_async" (uint64_t @-> ptr char @-> ocaml_bytes @-> ocaml_bytes @-> uint32_t @-> returning int)

let zk_groth16_prove_wait = fn "zk_groth16_prove_wait" (uint64_t @-> uint32_t @-> ocaml_bytes @-> returning int)

let zk_groth16_qap_eval =
  fn "zk_groth16_qap_eval" (uint64_t @-> ocaml_bytes @-> ocaml_bytes @-> ocaml_bytes @-> ocaml_bytes @-> returning int)

let zk_groth16_verify =
  fn "zk_groth16_verify"
    (ocaml_bytes @-> ocaml_bytes @-> ocaml_bytes @-> size_t @-> ocaml_bytes @-> ocaml_bytes @-> ocaml_bytes @-> ptr int @-> returning int)

(* the library's host pairing: prod_i e(P_i, Q_i) in its own GT encoding (groth16_mi355x.ml holds GT.to_bytes to it once per process) *)
let zk_pairing_product = fn "zk_pairing_product" (ocaml_bytes @-> ocaml_bytes @-> size_t @-> ocaml_bytes @-> returning int)

(* The verifiers in batches, on the device (include/zkmi355x.h, "the same three on the device"): one library call checks a list of proofs.
   ok: one byte per proof; status: one code per proof, or null. *)
let zk_pairing_product_many =
  fn "zk_pairing_product_many" (ocaml_bytes @-> ocaml_bytes @-> ptr uint64_t @-> uint32_t @-> ocaml_bytes @-> returning int)

let zk_groth16_verify_many =
  fn "zk_groth16_verify_many"
    (ocaml_bytes @-> ocaml_bytes @-> size_t @-> ocaml_bytes @-> ocaml_bytes @-> ocaml_bytes @-> ocaml_bytes @-> uint32_t @-> ocaml_bytes
   @-> ptr int32_t @-> returning int)

let zk_pinocchio_verify_many =
  fn "zk_pinocchio_verify_many"
    (ocaml_bytes @-> ocaml_bytes @-> size_t @-> ocaml_bytes @-> ocaml_bytes @-> uint32_t @-> ocaml_bytes @-> ptr int32_t @-> returning int)

let no_status : int32 ptr = from_voidp int32_t null

(* Verification keys resident on the device (include/zkmi355x.h, "verification keys resident on the device"): the key decoded and checked once,
   then one call per list of proofs that moves only the proofs and their public inputs.  Same ok / status as the _many calls. *)
let zk_groth16_vk_upload =
  fn "zk_groth16_vk_upload" (ocaml_bytes @-> ocaml_bytes @-> size_t @-> ocaml_bytes @-> ocaml_bytes @-> ptr uint64_t @-> returning int)

let zk_pinocchio_vk_upload = fn "zk_pinocchio_vk_upload" (ocaml_bytes @-> ocaml_bytes @-> size_t @-> ptr uint64_t @-> returning int)
let zk_vk_info = fn "zk_vk_info" (uint64_t @-> ptr int @-> ptr uint64_t @-> returning int)
let zk_vk_free = fn "zk_vk_free" (uint64_t @-> returning int)

let zk_groth16_verify_resident =
  fn "zk_groth16_verify_resident" (uint64_t @-> ocaml_bytes @-> ocaml_bytes @-> uint32_t @-> ocaml_bytes @-> ptr int32_t @-> returning int)

let zk_pinocchio_verify_resident =
  fn "zk_pinocchio_verify_resident" (uint64_t @-> ocaml_bytes @-> ocaml_bytes @-> uint32_t @-> ocaml_bytes @-> ptr int32_t @-> returning int)

(* One folded pairing equation for a whole list of proofs under a resident Groth16 key (include/zkmi355x.h, zk_groth16_verify_folded): rho holds 16
   bytes per proof, non-zero, drawn AFTER the proofs are fixed and unpredictable to whoever made them.  all_ok: 1 iff every proof is good. *)
let zk_groth16_verify_folded =
  fn "zk_groth16_verify_folded"
    (uint64_t @-> ocaml_bytes @-> ocaml_bytes @-> ocaml_bytes @-> uint32_t @-> ptr int @-> ptr int32_t @-> returning int)

(* the same stopped before the comparison: both sides as GT bytes and the two sums as points (the test suite's hook) *)
let zk_selftest_groth16_fold =
  fn "zk_selftest_groth16_fold"
    (uint64_t @-> ocaml_bytes @-> ocaml_bytes @-> ocaml_bytes @-> uint32_t @-> ocaml_bytes @-> ocaml_bytes @-> ocaml_bytes @-> ocaml_bytes
   @-> ptr int32_t @-> returning int)

(* The same question under a resident Pinocchio key (zk_pinocchio_verify_folded): rho holds FIVE coefficients per proof, one per equation of Verify.f,
   16 bytes each, every one non-zero, drawn AFTER the proofs are fixed and unpredictable to whoever made them. *)
let zk_pinocchio_verify_folded =
  fn "zk_pinocchio_verify_folded"
    (uint64_t @-> ocaml_bytes @-> ocaml_bytes @-> ocaml_bytes @-> uint32_t @-> ptr int @-> ptr int32_t @-> returning int)

(* the same stopped before the comparison: the left-hand side as GT bytes, the seven G1 sums and the three G2 sums as points (the test suite's hook) *)
let zk_selftest_pinocchio_fold =
  fn "zk_selftest_pinocchio_fold"
    (uint64_t @-> ocaml_bytes @-> ocaml_bytes @-> ocaml_bytes @-> uint32_t @-> ocaml_bytes @-> ocaml_bytes @-> ocaml_bytes @-> ptr int32_t
   @-> returning int)

(* The four verifiers on proofs in their compressed wire form (include/zkmi355x.h): 192 bytes per Groth16 proof, 480 per Pinocchio proof -- the
   to_compressed_bytes of the proof record's fields in declaration order -- decompressed on the device in the call that verifies them. *)
let zk_groth16_verify_resident_compressed =
  fn "zk_groth16_verify_resident_compressed"
    (uint64_t @-> ocaml_bytes @-> ocaml_bytes @-> uint32_t @-> ocaml_bytes @-> ptr int32_t @-> returning int)

let zk_pinocchio_verify_resident_compressed =
  fn "zk_pinocchio_verify_resident_compressed"
    (uint64_t @-> ocaml_bytes @-> ocaml_bytes @-> uint32_t @-> ocaml_bytes @-> ptr int32_t @-> returning int)

let zk_groth16_verify_folded_compressed =
  fn "zk_groth16_verify_folded_compressed"
    (uint64_t @-> ocaml_bytes @-> ocaml_bytes @-> ocaml_bytes @-> uint32_t @-> ptr int @-> ptr int32_t @-> returning int)

let zk_pinocchio_verify_folded_compressed =
  fn "zk_pinocchio_verify_folded_compressed"
    (uint64_t @-> ocaml_bytes @-> ocaml_bytes @-> ocaml_bytes @-> uint32_t @-> ptr int @-> ptr int32_t @-> returning int)

(* A batch of witnesses proved in one call, every proof out as its compressed wire bytes (include/zkmi355x.h): 192 bytes per Groth16 proof, 480 per
   Pinocchio proof -- the strings of the reference's proof record (groth16.ml:110-114, pinocchio.ml:195-208) back to back, what the *_compressed
   verifiers above take.  sols: the witnesses back to back, or null: the resident witness for every proof.  status: one code per proof. *)
let zk_groth16_prove_many_compressed =
  fn "zk_groth16_prove_many_compressed"
    (uint64_t @-> ptr char @-> ocaml_bytes @-> uint32_t @-> uint32_t @-> ocaml_bytes @-> ptr int32_t @-> returning int)

let zk_pinocchio_prove_many_compressed =
  fn "zk_pinocchio_prove_many_compressed"
    (uint64_t @-> ptr char @-> ocaml_bytes @-> uint32_t @-> uint32_t @-> ocaml_bytes @-> ptr int32_t @-> returning int)

(* the conversion launch of the two calls above on points the caller chooses (the test suite's hook) *)
let zk_selftest_proof_wire = fn "zk_selftest_proof_wire" (int @-> ocaml_bytes @-> ocaml_bytes @-> size_t @-> ocaml_bytes @-> returning int)

(* The body both protocols' prove_many_compressed share: `count` proofs of the resident witness, randomness back to back in `rnd`, `size` wire bytes per
   proof.  The first proof that failed raises what the single call raises (check); otherwise the proofs' wire bytes, one string each. *)
let prove_many_compressed stub (h : Unsigned.UInt64.t) ~(rnd : bytes) ~(count : int) ~(size : int) : bytes list =
  if count = 0 then []
  else begin
    let out = Bytes.create (size * count) in
    let status = CArray.make int32_t ~initial:0l count in
    check (stub h null_bytes (bytes_start rnd) (u32 count) (u32 0) (bytes_start out) (CArray.start status));
    CArray.iter (fun st -> check (Int32.to_int st)) status;
    List.init count (fun i -> Bytes.sub out (size * i) size)
  end

let vk_free (h : Unsigned.UInt64.t) = ignore (zk_vk_free h)

let groth16_upload ~n ~m (l : matrix) (r : matrix) (o : matrix) ~(mid : bytes) ~(g1 : bytes) ~(g2 : bytes) : Unsigned.UInt64.t =
  let h = allocate uint64_t Unsigned.UInt64.zero in
  check
    (zk_groth16_pk_upload (u32 n) (u32 m) (addr l.c) (addr r.c) (addr o.c) (bytes_start mid) (bytes_start g1)
       (sz (Bytes.length g1 / 96))
       (bytes_start g2)
       (sz (Bytes.length g2 / 192))
       h);
  !@h

(* ------------------------------------------------------------------ Pinocchio Protocol 2: pinocchio.ml:37-60,210-248,427-514 *)

let zk_pinocchio_pk_upload =
  fn "zk_pinocchio_pk_upload"
    (uint32_t @-> uint32_t @-> ptr csr @-> ptr csr @-> ptr csr @-> ocaml_bytes @-> ocaml_bytes @-> size_t @-> ocaml_bytes @-> size_t
   @-> ptr uint64_t @-> returning int)

let zk_pinocchio_pk_derive_lagrange = fn "zk_pinocchio_pk_derive_lagrange" (uint64_t @-> returning int)
let zk_pinocchio_pk_free = fn "zk_pinocchio_pk_free" (uint64_t @-> returning int)

let zk_pinocchio_prove =
  fn "zk_pinocchio_prove"
    (uint64_t @-> ocaml_bytes @-> ocaml_bytes @-> ocaml_bytes @-> ocaml_bytes @-> ocaml_bytes @-> returning int)

let zk_pinocchio_reserve_slots = fn "zk_pinocchio_reserve_slots" (uint64_t @-> uint32_t @-> returning int)
let zk_pinocchio_set_witness = fn "zk_pinocchio_set_witness" (uint64_t @-> ocaml_bytes @-> returning int)

let zk_pinocchio_prove_async =
  fn "zk_pinocchio_prove_async"
    (uint64_t @-> ptr char @-> ocaml_bytes @-> ocaml_bytes @-> ocaml_bytes @-> uint32_t @-> returning int)

let zk_pinocchio_prove_wait = fn "zk_pinocchio_prove_wait" (uint64_t @-> uint32_t @-> ocaml_bytes @-> returning int)

let zk_pinocchio_verify =
  fn "zk_pinocchio_verify" (ocaml_bytes @-> ocaml_bytes @-> ocaml_bytes @-> size_t @-> ocaml_bytes @-> ptr int @-> returning int)

(* zk_pinocchio_pk_upload plus the stored h bases [lambda_t(s)] (n-1) | [Z(s)] of a derived key (header): the key starts in its derived form *)
let zk_pinocchio_pk_upload_lagrange =
  fn "zk_pinocchio_pk_upload_lagrange"
    (uint32_t @-> uint32_t @-> ptr csr @-> ptr csr @-> ptr csr @-> ocaml_bytes @-> ocaml_bytes @-> size_t @-> ocaml_bytes @-> size_t
   @-> ocaml_bytes @-> ptr uint64_t @-> returning int)

(* ---- keys and base lists in WIRE form (include/zkmi355x.h, "keys and base lists in WIRE form"): the compressed strings of the reference's JSON
   (to_compressed_bytes, curve.ml:199-219), 48 B per G1 point and 96 B per G2 point, decoded and checked on the device.  The identity is C0 00 .. 00
   only; the library returns the verdict of the first bad point (Not_on_curve / Invalid_argument through `check`). *)
let zk_groth16_pk_upload_compressed =
  fn "zk_groth16_pk_upload_compressed"
    (uint32_t @-> uint32_t @-> ptr csr @-> ptr csr @-> ptr csr @-> ocaml_bytes @-> ocaml_bytes @-> size_t @-> ocaml_bytes @-> size_t
   @-> uint32_t @-> ptr uint64_t @-> returning int)

let zk_pinocchio_pk_upload_compressed =
  fn "zk_pinocchio_pk_upload_compressed"
    (uint32_t @-> uint32_t @-> ptr csr @-> ptr csr @-> ptr csr @-> ocaml_bytes @-> ocaml_bytes @-> size_t @-> ocaml_bytes @-> size_t
   @-> ptr char @-> ptr uint64_t @-> returning int)

let zk_bases_upload_compressed = fn "zk_bases_upload_compressed" (int @-> ocaml_bytes @-> size_t @-> ptr uint64_t @-> returning int)

let zk_groth16_pool_points_compressed =
  fn "zk_groth16_pool_points_compressed" (uint64_t @-> int @-> ptr char @-> size_t @-> ptr size_t @-> returning int)

let zk_pinocchio_pool_points_compressed =
  fn "zk_pinocchio_pool_points_compressed" (uint64_t @-> int @-> ptr char @-> size_t @-> ptr size_t @-> returning int)

(* form: 0 = the tau powers of the reference's key, 1 = the Lagrange-form pools: the header's key forms *)
let groth16_upload_compressed ?(form = 0) ~n ~m (l : matrix) (r : matrix) (o : matrix) ~(mid : bytes) ~(g1 : bytes) ~(g2 : bytes) : Unsigned.UInt64.t =
  let h = allocate uint64_t Unsigned.UInt64.zero in
  check
    (zk_groth16_pk_upload_compressed (u32 n) (u32 m) (addr l.c) (addr r.c) (addr o.c) (bytes_start mid) (bytes_start g1)
       (sz (Bytes.length g1 / 48))
       (bytes_start g2)
       (sz (Bytes.length g2 / 96))
       (u32 form) h);
  !@h

(* h_lagrange: the n stored h bases of a derived key (48 B each); without them the key starts as uploaded *)
let pinocchio_upload_compressed ?h_lagrange ~n ~m (l : matrix) (r : matrix) (o : matrix) ~(mid : bytes) ~(g1 : bytes) ~(g2 : bytes) : Unsigned.UInt64.t =
  let h = allocate uint64_t Unsigned.UInt64.zero in
  let hl = Option.map carray_of_bytes h_lagrange in
  check
    (zk_pinocchio_pk_upload_compressed (u32 n) (u32 m) (addr l.c) (addr r.c) (addr o.c) (bytes_start mid) (bytes_start g1)
       (sz (Bytes.length g1 / 48))
       (bytes_start g2)
       (sz (Bytes.length g2 / 96))
       (match hl with Some a -> CArray.start a | None -> null_bytes)
       h);
  !@h

(* a resident base list from its wire bytes (zk_bases_upload_compressed) *)
let resident_upload_compressed ~(g2 : bool) (points : bytes) : Unsigned.UInt64.t =
  let h = allocate uint64_t Unsigned.UInt64.zero in
  check (zk_bases_upload_compressed (if g2 then 1 else 0) (bytes_start points) (sz (Bytes.length points / if g2 then 96 else 48)) h);
  !@h

(* a resident pool in wire form: what *_upload_compressed takes back (the key cache: derive once, store, reload) *)
let pool_points_compressed stub (h : Unsigned.UInt64.t) ~(pool : int) ~(point_bytes : int) : bytes =
  let cnt = allocate size_t Unsigned.Size_t.zero in
  check (stub h pool null_bytes Unsigned.Size_t.zero cnt);          (* out = NULL: the count alone *)
  let len = Unsigned.Size_t.to_int !@cnt * point_bytes in
  let out = CArray.make char (max 1 len) in
  check (stub h pool (CArray.start out) !@cnt cnt);
  Bytes.init len (fun i -> CArray.get out i)

(* The key as a whole against its circuit and, when given, its verification key (include/zkmi355x.h, "the key as a whole"): vk_g1, vk_g2 and seed may be
   null.  failed: the mask of the relations that do not hold (the header's ZK_KEYCHK bits), 0 for a well-formed key. *)
let zk_groth16_key_check =
  fn "zk_groth16_key_check" (uint64_t @-> ptr char @-> size_t @-> ptr char @-> ptr char @-> ptr uint32_t @-> returning int)

(* the bits of the mask, in bit order, under their names *)
let keychk_names = [ (1, "generators"); (2, "tau_g1"); (4, "tau_g2"); (8, "beta"); (16, "delta"); (32, "h_bases"); (64, "l"); (128, "gamma") ]

(* vk: (one1 | ltgm_io, one2 | gm | d) as uncompressed bytes, or None: the key against its circuit alone.  seed: 32 bytes the CALLER drew from a
   cryptographic generator after the key's bytes were fixed (the header's contract); None: the library draws them.  Returns the mask. *)
let key_check_call stub ?vk ?seed (h : Unsigned.UInt64.t) : int =
  let failed = allocate uint32_t Unsigned.UInt32.zero in
  let arr = Option.map carray_of_bytes in
  let v1 = arr (Option.map fst vk) and v2 = arr (Option.map snd vk) and sd = arr seed in
  let start = function Some a -> CArray.start a | None -> null_bytes in
  let n_io = match vk with Some (g1, _) -> (Bytes.length g1 / 96) - 1 | None -> 0 in
  check (stub h (start v1) (sz n_io) (start v2) (start sd) failed);
  Unsigned.UInt32.to_int !@failed

let groth16_key_check ?vk ?seed (h : Unsigned.UInt64.t) : int = key_check_call zk_groth16_key_check ?vk ?seed h

(* The same question for a handle in Lagrange form (include/zkmi355x.h, "a Lagrange-form key as a whole"): pools loaded with form = key_form_lagrange,
   generated in that form or derived on the device.  The same arguments, the same bits; a tau-power handle is refused. *)
let zk_groth16_key_check_lagrange =
  fn "zk_groth16_key_check_lagrange" (uint64_t @-> ptr char @-> size_t @-> ptr char @-> ptr char @-> ptr uint32_t @-> returning int)

let groth16_key_check_lagrange ?vk ?seed (h : Unsigned.UInt64.t) : int = key_check_call zk_groth16_key_check_lagrange ?vk ?seed h

(* A delta contribution to the resident key (include/zkmi355x.h, "a delta contribution to a resident key"): d1, d2 times delta', the tail of the G1 pool
   times 1 / delta', new window tables, all on the device.  dmul: delta', 32 canonical bytes.  Returns (d1 before | d1 after, [delta']_2, d2 after): the
   link of the two keys and the d of the new verification key, uncompressed. *)
let zk_groth16_pk_contribute =
  fn "zk_groth16_pk_contribute" (uint64_t @-> ptr char @-> ptr char @-> ptr char @-> ptr char @-> returning int)

let groth16_pk_contribute (h : Unsigned.UInt64.t) ~(dmul : bytes) : bytes * bytes * bytes =
  let d = carray_of_bytes dmul in
  let link = CArray.make char 192 and dg2 = CArray.make char 192 and vkd = CArray.make char 192 in
  check (zk_groth16_pk_contribute h (CArray.start d) (CArray.start link) (CArray.start dg2) (CArray.start vkd));
  let out a = Bytes.init 192 (fun i -> CArray.get a i) in
  (out link, out dg2, out vkd)

(* A phase-1 string as a whole (include/zkmi355x.h, "a phase-1 string as a whole"): srs_g1 = tau1[N1] | alpha_tau1[NAB] | beta_tau1[NAB], srs_g2 =
   beta2 | tau2[N2], uncompressed, of the caller's lengths.  The check gives a mask (0: well formed); seed as for key_check_call.  The contribution
   multiplies the string by mul = alpha' | beta' | tau' (96 canonical bytes) and returns (srs_g1, srs_g2, link_g1, link_g2). *)
let zk_groth16_srs_check =
  fn "zk_groth16_srs_check" (ptr char @-> size_t @-> size_t @-> ptr char @-> size_t @-> ptr char @-> ptr uint32_t @-> returning int)

let zk_groth16_srs_contribute =
  fn "zk_groth16_srs_contribute"
    (ptr char @-> size_t @-> size_t @-> ptr char @-> size_t @-> ptr char @-> ptr char @-> ptr char @-> ptr char @-> ptr char @-> returning int)

(* the bits of the check's mask under their names, in bit order (name first: the pairs of keychk_names above are the key check's alone) *)
let srschk_names = [ ("generators", 1); ("tau_g1", 2); ("tau_g2", 4); ("alpha", 8); ("beta", 16); ("trivial", 32) ]

let groth16_srs_check ?seed ~(srs_g1 : bytes) ~tau1_points ~ab_points ~(srs_g2 : bytes) ~tau2_points () : int =
  let failed = allocate uint32_t Unsigned.UInt32.zero in
  let s1 = carray_of_bytes srs_g1 and s2 = carray_of_bytes srs_g2 and sd = Option.map carray_of_bytes seed in
  let start = function Some a -> CArray.start a | None -> null_bytes in
  check (zk_groth16_srs_check (CArray.start s1) (sz tau1_points) (sz ab_points) (CArray.start s2) (sz tau2_points) (start sd) failed);
  Unsigned.UInt32.to_int !@failed

let groth16_srs_contribute ~(srs_g1 : bytes) ~tau1_points ~ab_points ~(srs_g2 : bytes) ~tau2_points ~(mul : bytes) : bytes * bytes * bytes * bytes =
  let s1 = carray_of_bytes srs_g1 and s2 = carray_of_bytes srs_g2 and k = carray_of_bytes mul in
  let n1 = Bytes.length srs_g1 and n2 = Bytes.length srs_g2 in
  let o1 = CArray.make char n1 and o2 = CArray.make char n2 and l1 = CArray.make char (6 * 96) and l2 = CArray.make char (3 * 192) in
  check
    (zk_groth16_srs_contribute (CArray.start s1) (sz tau1_points) (sz ab_points) (CArray.start s2) (sz tau2_points) (CArray.start k) (CArray.start o1)
       (CArray.start o2) (CArray.start l1) (CArray.start l2));
  let out a len = Bytes.init len (fun i -> CArray.get a i) in
  (out o1 n1, out o2 n2, out l1 (6 * 96), out l2 (3 * 192))

let pinocchio_upload ~n ~m (l : matrix) (r : matrix) (o : matrix) ~(mid : bytes) ~(g1 : bytes) ~(g2 : bytes) : Unsigned.UInt64.t =
  let h = allocate uint64_t Unsigned.UInt64.zero in
  check
    (zk_pinocchio_pk_upload (u32 n) (u32 m) (addr l.c) (addr r.c) (addr o.c) (bytes_start mid) (bytes_start g1)
       (sz (Bytes.length g1 / 96))
       (bytes_start g2)
       (sz (Bytes.length g2 / 192))
       h);
  !@h

(* ------------------------------------------------------------------ N GPUs, one process per GPU (header, "point-sharded multi-GPU prove") *)

let zk_groth16_pk_shard = fn "zk_groth16_pk_shard" (uint64_t @-> uint32_t @-> uint32_t @-> returning int)

let zk_groth16_prove_partial_async =
  fn "zk_groth16_prove_partial_async" (uint64_t @-> ocaml_bytes @-> ocaml_bytes @-> ocaml_bytes @-> uint32_t @-> returning int)

let zk_groth16_prove_partial_wait_device =
  fn "zk_groth16_prove_partial_wait_device" (uint64_t @-> uint32_t @-> ptr void @-> returning int)

let zk_groth16_combine_device =
  fn "zk_groth16_combine_device" (ptr void @-> size_t @-> uint32_t @-> ocaml_bytes @-> returning int)

let zk_device_malloc = fn "zk_device_malloc" (size_t @-> ptr (ptr void) @-> returning int)
let zk_device_free = fn "zk_device_free" (ptr void @-> returning int)
