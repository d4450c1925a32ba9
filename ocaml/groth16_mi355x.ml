(* groth16_mi355x.ml -- seam 2: the body of src/groth16/groth16.ml with the prover on the MI355X.

   Install as src/groth16/groth16.ml; groth16.mli stays byte-identical (module Make(C : Curve.S) : Protocol.S with ...).
   The one change outside src/groth16: `module type G` of src/lib/zk/curve.ml / curve.mli gains
       val to_bytes : t -> bytes
       val of_bytes_exn : bytes -> t
   which every instance already has (they come with opam bls12-381's Fr, G1, G2, GT) -- a functor over an abstract
   Curve.S has no other way to hand group elements to a C library (ocaml/README.md).

   What is replaced (reference lines):
     prove   groth16.ml:235-237 + Base.prove :123-161 + sum_apply_powers :116-121 + QAP.eval (QAP.ml:120-135)
             -> one call zk_groth16_prove on a key uploaded once; r and s are drawn HERE, r first (:124-125)
     keygen  groth16.ml:227-233 + setup :45-108
             -> one call zk_groth16_keygen: the trapdoor is drawn HERE in the reference's order (:51-55), exponents and points are the device's;
                the key's bytes and a live handle in Lagrange form come back (a multi-device list: the bytes, then the ordinary upload)
     verify  groth16.ml:163-173 -> unchanged in substance: three pairings of the host's own Pairing
             verify_many (an extra): a list of proofs under one key -> one call zk_groth16_verify_many, the pairings on the device
             Verifier (an extra): the key resident on the device, create / verify_many / verify_all / free -> a call moves only proofs and public inputs;
                       verify_all asks one folded pairing equation about the whole list
   The records and their yojson are the reference's (groth16.ml:24-43,110-114): the JSON of keys and proofs is the wire format. *)

open Zukelang
open Yojson_conv

module Make (C : Curve.S) = struct
  open C
  module Circuit = Circuit.Make (Fr)
  module QAP = QAP.Make (Fr)
  module Poly = QAP.Polynomial

  type f = Fr.t
  type circuit = Circuit.t
  type qap = QAP.t

  type pkey =
    { a : G1.t;
      d1 : G1.t;
      ti1 : G1.t list;
      ltd_mid : G1.t Var.Map.t;
      tiztd : G1.t list;
      b1 : G1.t;
      b2 : G2.t;
      d2 : G2.t;
      ti2 : G2.t list
    }
  [@@deriving yojson]

  type vkey =
    { one1 : G1.t;
      ltgm_io : G1.t Var.Map.t;
      one2 : G2.t;
      gm : G2.t;
      d : G2.t;
      ab : GT.t
    }
  [@@deriving yojson]

  type proof = { a : G1.t; b : G2.t; c : G1.t } [@@deriving yojson]

  (* ---------------------------------------------------------------- bytes *)

  let fr_bytes (xs : Fr.t list) = Mi355x.cat (List.map Fr.to_bytes xs)
  let g1_bytes (ps : G1.t list) = Mi355x.cat (List.map G1.to_bytes ps)
  let g2_bytes (ps : G2.t list) = Mi355x.cat (List.map G2.to_bytes ps)
  let g1_at b i = G1.of_bytes_exn (Bytes.sub b (96 * i) 96)
  let g2_at b i = G2.of_bytes_exn (Bytes.sub b (192 * i) 192)
  let values m = List.map snd (Var.Map.bindings m)

  (* ---------------------------------------------------------------- the circuit as three sparse matrices
     Rows = gates in Gate.Set.elements order (the ids QAP.build gives them, QAP.ml:22), columns = variables in Var.Map key
     order, entry = the coefficient QAP.build reads off the gate (QAP.ml:30-52). *)

  let index_of_vars (vars : Var.t list) : int Var.Map.t = Var.Map.of_list (List.mapi (fun i v -> (v, i)) vars)

  let matrices_of_gates (index : int Var.Map.t) (gates : Circuit.Gate.Set.t) =
    let rows sel =
      List.map
        (fun g -> List.map (fun (v, coeff) -> (Var.Map.find v index, Fr.to_bytes coeff)) (Var.Map.bindings (sel g)))
        (Circuit.Gate.Set.elements gates)
    in
    ( Mi355x.matrix_of_rows (rows (fun (g : Circuit.Gate.t) -> g.l)),
      Mi355x.matrix_of_rows (rows (fun (g : Circuit.Gate.t) -> g.r)),
      Mi355x.matrix_of_rows (rows (fun (g : Circuit.Gate.t) -> g.lhs)) )

  (* Without the circuit (a key read back from JSON, proved against a QAP): the coefficient of variable k in gate g is
     v_k(g) -- what QAP.decompile recovers (QAP.ml:96-118).  O(m n^2) field operations; only for sizes at which a dense
     QAP.t exists at all. *)
  let matrices_of_qap (index : int Var.Map.t) (qap : qap) n =
    let rows (polys : Poly.t Var.Map.t) =
      List.init n (fun g ->
          let x = Fr.of_int g in
          List.filter_map
            (fun (v, p) ->
              let coeff = Poly.apply p x in
              if Fr.(coeff = zero) then None else Some (Var.Map.find v index, Fr.to_bytes coeff))
            (Var.Map.bindings polys))
    in
    (Mi355x.matrix_of_rows (rows qap.v), Mi355x.matrix_of_rows (rows qap.w), Mi355x.matrix_of_rows (rows qap.y))

  (* ---------------------------------------------------------------- uploaded keys
     pkey is [@@deriving yojson], so the device handle cannot be a field of it.  It lives in a side table keyed by the
     (physically equal) pkey value; the entry dies with the key and the finaliser frees the device copy. *)

  module Handles = Ephemeron.K1.Make (struct
    type t = pkey

    let equal = ( == )
    let hash (k : pkey) = List.length k.ti1
  end)

  let handles : Unsigned.UInt64.t Handles.t = Handles.create 8

  (* set before the first prove of a key that will prove many times: the library then derives the key's Lagrange form on
     the device once (zk_groth16_pk_derive_lagrange; pays off after a few thousand proofs, header) *)
  let derive_lagrange_on_upload = ref false

  let upload (vars : Var.t list) (l, r, o) n (pkey : pkey) : Unsigned.UInt64.t =
    let var_at = Array.of_list vars in
    let m = Array.length var_at in
    let mid = Bytes.init m (fun i -> if Var.Map.mem var_at.(i) pkey.ltd_mid then '\001' else '\000') in
    (* declaration order of groth16.ml:24-34 per group, as include/zkmi355x.h lays it out *)
    let g1 = g1_bytes ((pkey.a :: pkey.d1 :: pkey.b1 :: pkey.ti1) @ pkey.tiztd @ values pkey.ltd_mid) in
    let g2 = g2_bytes (pkey.b2 :: pkey.d2 :: pkey.ti2) in
    let h = Mi355x.groth16_upload ~n ~m l r o ~mid ~g1 ~g2 in
    if !derive_lagrange_on_upload then Mi355x.(check (zk_groth16_pk_derive_lagrange h));
    Gc.finalise (fun _ -> ignore (Mi355x.zk_groth16_pk_free h)) pkey;
    Handles.replace handles pkey h;
    h

  (* a key whose bytes exist on the host -- read from JSON, or generated while the device list had several entries -- enters the library here *)
  let register = upload

  (* The same from the record's COMPRESSED strings as they stand in the JSON (zk_groth16_pk_upload_compressed): g1 = a | d1 | b1 | ti1 | tiztd | ltd_mid
     and g2 = b2 | d2 | ti2, 48 / 96 B per point, decoded and checked on the device -- no of_compressed_bytes_exn per point on the host and no
     uncompressed copy.  lagrange: the strings are the pools of a derived key (Mi355x.pool_points_compressed after zk_groth16_pk_derive_lagrange).
     The handle is registered under pkey like any other. *)
  let upload_compressed ?(lagrange = false) (vars : Var.t list) (l, r, o) n (pkey : pkey) ~(g1 : bytes) ~(g2 : bytes) : Unsigned.UInt64.t =
    let var_at = Array.of_list vars in
    let m = Array.length var_at in
    let mid = Bytes.init m (fun i -> if Var.Map.mem var_at.(i) pkey.ltd_mid then '\001' else '\000') in
    let h = Mi355x.groth16_upload_compressed ~form:(if lagrange then 1 else 0) ~n ~m l r o ~mid ~g1 ~g2 in
    Gc.finalise (fun _ -> ignore (Mi355x.zk_groth16_pk_free h)) pkey;
    Handles.replace handles pkey h;
    h

  let pool_compressed (h : Unsigned.UInt64.t) ~(group : int) : bytes =
    Mi355x.pool_points_compressed Mi355x.zk_groth16_pool_points_compressed h ~pool:group ~point_bytes:(if group = 1 then 48 else 96)

  let handle_of (qap : qap) (pkey : pkey) =
    match Handles.find_opt handles pkey with
    | Some h -> h
    | None ->
        let vars = List.map fst (Var.Map.bindings qap.v) in
        let n = Poly.degree qap.target in
        upload vars (matrices_of_qap (index_of_vars vars) qap n) n pkey

  (* ---------------------------------------------------------------- keygen *)

  let keygen rng (circuit : circuit) (qap : qap) : pkey * vkey =
    let n = Poly.degree qap.target in
    let alpha = Fr.gen rng in
    let beta = Fr.gen rng in
    let gamma = Fr.gen rng in
    let delta = Fr.gen rng in
    let tau = Fr.gen rng in
    (* ONE library call (zk_groth16_keygen): every exponent of groth16.ml:59-90 is computed on the device from the trapdoor and the circuit's
       rows, every point by the fixed-base kernel.  The bytes that come back are the key in the reference's format; the handle that comes back
       with them already holds the key's Lagrange form (the fast prover's), so nothing is sent or derived a second time -- on a device list of one
       entry; on a longer list no handle is offered and the bytes are registered like a key read from JSON (below). *)
    let vars = List.map fst (Var.Map.bindings qap.v) in
    let m = List.length vars in
    let is_mid v = Var.Set.mem v circuit.Circuit.mids in
    let mids = List.filter is_mid vars and ios = List.filter (fun v -> not (is_mid v)) vars in
    let io_set = Var.Set.union circuit.Circuit.inputs_public circuit.Circuit.outputs in
    if not (List.for_all (fun v -> Var.Set.mem v io_set) ios) then assert false;
    let mid = Mi355x.cat (List.map (fun v -> Bytes.make 1 (if is_mid v then '\001' else '\000')) vars) in
    let n_ti = n + 2 and n_tiz = max (n - 1) 0 and n_mid = List.length mids and n_io = List.length ios in
    let l, r, o = matrices_of_gates (index_of_vars vars) circuit.Circuit.gates in
    let p1, p2, v1, v2, h =
      Mi355x.keygen_call Mi355x.zk_groth16_keygen ~n ~m l r o ~mid
        ~toxic:(fr_bytes [ alpha; beta; gamma; delta; tau ])
        ~form:Mi355x.key_form_lagrange
        ~g1_points:(3 + n_ti + n_tiz + n_mid)
        ~g2_points:(2 + n_ti) ~vk1_points:(1 + n_io) ~vk2_points:3
    in
    let take b at off count = List.init count (fun i -> at b (off + i)) in
    let rekey ks points = Var.Map.of_list (List.combine ks points) in
    let pkey : pkey =
      { a = g1_at p1 0;
        d1 = g1_at p1 1;
        b1 = g1_at p1 2;
        ti1 = take p1 g1_at 3 n_ti;
        tiztd = take p1 g1_at (3 + n_ti) n_tiz;
        ltd_mid = rekey mids (take p1 g1_at (3 + n_ti + n_tiz) n_mid);
        b2 = g2_at p2 0;
        d2 = g2_at p2 1;
        ti2 = take p2 g2_at 2 n_ti
      }
    in
    let vkey : vkey =
      { one1 = g1_at v1 0;
        ltgm_io = rekey ios (take v1 g1_at 1 n_io);
        one2 = g2_at v2 0;
        gm = g2_at v2 1;
        d = g2_at v2 2;
        ab = Pairing.pairing pkey.a pkey.b2
      }
    in
    (match h with
    | Some h ->
        Gc.finalise (fun _ -> ignore (Mi355x.zk_groth16_pk_free h)) pkey;
        Handles.replace handles pkey h
    | None ->
        (* a device list of several entries (Mi355x.use_all_devices): the generated bytes go through zk_groth16_pk_upload, which shards the key over
           the list behind one handle; derive_lagrange_on_upload applies to it as to any uploaded key *)
        ignore (register vars (l, r, o) n pkey));
    (pkey, vkey)

  (* ---------------------------------------------------------------- specialize
     A phase-1 string specialised to the circuit on the device (zk_groth16_pk_specialize): the keys `keygen` would give for the trapdoor
     (alpha, beta, 1, 1, tau) from [tau^i]_1 (max (n+2) (2n-1) of them), [alpha tau^i]_1, [beta tau^i]_1 (n each), [beta]_2 and [tau^i]_2 (n+2) --
     nobody knows the trapdoor.  The lists must have exactly those lengths (Mi355x.groth16_srs_sizes).  The call trusts the string: run check_key
     with the returned vkey on the result, then contribute. *)
  let specialize (circuit : circuit) (qap : qap) ~(tau1 : G1.t list) ~(alpha_tau1 : G1.t list) ~(beta_tau1 : G1.t list) ~(beta2 : G2.t)
      ~(tau2 : G2.t list) : pkey * vkey =
    let n = Poly.degree qap.target in
    let vars = List.map fst (Var.Map.bindings qap.v) in
    let m = List.length vars in
    let is_mid v = Var.Set.mem v circuit.Circuit.mids in
    let mids = List.filter is_mid vars and ios = List.filter (fun v -> not (is_mid v)) vars in
    let mid = Mi355x.cat (List.map (fun v -> Bytes.make 1 (if is_mid v then '\001' else '\000')) vars) in
    let n_ti = n + 2 and n_tiz = max (n - 1) 0 and n_mid = List.length mids and n_io = List.length ios in
    let l, r, o = matrices_of_gates (index_of_vars vars) circuit.Circuit.gates in
    let p1, p2, v1, v2, h =
      Mi355x.specialize_call ~n ~m l r o ~mid
        ~srs_g1:(Mi355x.cat [ g1_bytes tau1; g1_bytes alpha_tau1; g1_bytes beta_tau1 ])
        ~srs_g2:(Mi355x.cat [ G2.to_bytes beta2; g2_bytes tau2 ])
        ~form:Mi355x.key_form_lagrange
        ~g1_points:(3 + n_ti + n_tiz + n_mid)
        ~g2_points:(2 + n_ti) ~vk1_points:(1 + n_io) ~vk2_points:3
    in
    let take b at off count = List.init count (fun i -> at b (off + i)) in
    let rekey ks points = Var.Map.of_list (List.combine ks points) in
    let pkey : pkey =
      { a = g1_at p1 0;
        d1 = g1_at p1 1;
        b1 = g1_at p1 2;
        ti1 = take p1 g1_at 3 n_ti;
        tiztd = take p1 g1_at (3 + n_ti) n_tiz;
        ltd_mid = rekey mids (take p1 g1_at (3 + n_ti + n_tiz) n_mid);
        b2 = g2_at p2 0;
        d2 = g2_at p2 1;
        ti2 = take p2 g2_at 2 n_ti
      }
    in
    let vkey : vkey =
      { one1 = g1_at v1 0;
        ltgm_io = rekey ios (take v1 g1_at 1 n_io);
        one2 = g2_at v2 0;
        gm = g2_at v2 1;
        d = g2_at v2 2;
        ab = Pairing.pairing pkey.a pkey.b2
      }
    in
    (match h with
    | Some h ->
        Gc.finalise (fun _ -> ignore (Mi355x.zk_groth16_pk_free h)) pkey;
        Handles.replace handles pkey h
    | None -> ignore (register vars (l, r, o) n pkey));
    (pkey, vkey)

  (* ---------------------------------------------------------------- srs_check, srs_contribute
     The two stations before `specialize` (zk_groth16_srs_check, zk_groth16_srs_contribute), on a string of ANY lengths: check a long string once,
     then cut it to circuits.  srs_check returns the names of the relations that do not hold ([] = well formed); seed as for check_key.
     srs_contribute multiplies the string by (alpha', beta', tau') on the device and returns the new lists with the link
     (tau1[1], alpha_tau1[0], beta_tau1[0] before | after each; [tau']_2 | [alpha']_2 | [beta']_2), uncompressed.  It trusts the string: check
     before and after. *)
  let srs_bytes ~tau1 ~alpha_tau1 ~beta_tau1 ~beta2 ~tau2 =
    if List.length alpha_tau1 <> List.length beta_tau1 then invalid_arg "srs: alpha_tau1 and beta_tau1 have one length";
    (Mi355x.cat [ g1_bytes tau1; g1_bytes alpha_tau1; g1_bytes beta_tau1 ], Mi355x.cat [ G2.to_bytes beta2; g2_bytes tau2 ])

  let srs_check ?(seed : bytes option) ~(tau1 : G1.t list) ~(alpha_tau1 : G1.t list) ~(beta_tau1 : G1.t list) ~(beta2 : G2.t) ~(tau2 : G2.t list) () :
      string list =
    let srs_g1, srs_g2 = srs_bytes ~tau1 ~alpha_tau1 ~beta_tau1 ~beta2 ~tau2 in
    let mask =
      Mi355x.groth16_srs_check ?seed ~srs_g1 ~tau1_points:(List.length tau1) ~ab_points:(List.length alpha_tau1) ~srs_g2 ~tau2_points:(List.length tau2) ()
    in
    List.filter_map (fun (name, bit) -> if mask land bit <> 0 then Some name else None) Mi355x.srschk_names

  let srs_contribute ~(alpha_mul : Fr.t) ~(beta_mul : Fr.t) ~(tau_mul : Fr.t) ~(tau1 : G1.t list) ~(alpha_tau1 : G1.t list) ~(beta_tau1 : G1.t list)
      ~(beta2 : G2.t) ~(tau2 : G2.t list) : (G1.t list * G1.t list * G1.t list * G2.t * G2.t list) * bytes * bytes =
    let srs_g1, srs_g2 = srs_bytes ~tau1 ~alpha_tau1 ~beta_tau1 ~beta2 ~tau2 in
    let n1 = List.length tau1 and nab = List.length alpha_tau1 and n2 = List.length tau2 in
    let o1, o2, link_g1, link_g2 =
      Mi355x.groth16_srs_contribute ~srs_g1 ~tau1_points:n1 ~ab_points:nab ~srs_g2 ~tau2_points:n2 ~mul:(fr_bytes [ alpha_mul; beta_mul; tau_mul ])
    in
    let take b at off count = List.init count (fun i -> at b (off + i)) in
    ((take o1 g1_at 0 n1, take o1 g1_at n1 nab, take o1 g1_at (n1 + nab) nab, g2_at o2 0, take o2 g2_at 1 n2), link_g1, link_g2)

  (* ---------------------------------------------------------------- prove *)

  let prove rng (qap : qap) (pkey : pkey) (sol : f Var.Map.t) : proof =
    let handle = handle_of qap pkey in
    let r = Fr.gen rng in
    let s = Fr.gen rng in
    (* the reference folds over Dom(sol) and looks every key up in the QAP (`#!`: assert false when absent, var.ml:71-78) *)
    if not (Var.Set.equal (Var.Map.domain sol) (Var.Map.domain qap.v)) then assert false;
    let out = Bytes.create 384 in
    Mi355x.(
      check
        (zk_groth16_prove handle
           (bytes_start (fr_bytes (values sol)))
           (bytes_start (Fr.to_bytes r))
           (bytes_start (Fr.to_bytes s))
           (bytes_start out)));
    { a = g1_at out 0; b = G2.of_bytes_exn (Bytes.sub out 96 192); c = G1.of_bytes_exn (Bytes.sub out 288 96) }

  (* Throughput form: several proofs of one key in flight (header, zk_groth16_prove_async).  `jobs` = the (r, s) pairs,
     drawn by the caller in the reference's order; the witness is uploaded once. *)
  let prove_many (qap : qap) (pkey : pkey) (sol : f Var.Map.t) (jobs : (Fr.t * Fr.t) list) : proof list =
    let handle = handle_of qap pkey in
    let slots = 14 in
    Mi355x.(check (zk_groth16_reserve_slots handle (u32 slots)));
    Mi355x.(check (zk_groth16_set_witness handle (bytes_start (fr_bytes (values sol)))));
    let collect slot =
      let out = Bytes.create 384 in
      Mi355x.(check (zk_groth16_prove_wait handle (u32 slot) (bytes_start out)));
      ({ a = g1_at out 0; b = G2.of_bytes_exn (Bytes.sub out 96 192); c = G1.of_bytes_exn (Bytes.sub out 288 96) } : proof)
    in
    let rec go i pending acc = function
      | [] -> List.rev_append acc (List.map collect (List.rev pending))
      | (r, s) :: rest ->
          let slot = i mod slots in
          let acc, pending =
            if List.length pending = slots then
              match List.rev pending with
              | oldest :: others -> (collect oldest :: acc, List.rev others)
              | [] -> (acc, pending)
            else (acc, pending)
          in
          Mi355x.(
            check
              (zk_groth16_prove_async handle null_bytes (bytes_start (Fr.to_bytes r)) (bytes_start (Fr.to_bytes s)) (u32 slot)));
          go (i + 1) (slot :: pending) acc rest
    in
    go 0 [] [] jobs

  (* The same batch in ONE library call, the proofs as their wire bytes (zk_groth16_prove_many_compressed): a 48 | b 96 | c 48 per proof, the strings of
     proof_to_yojson (groth16.ml:110-114) and what Resident.verify_many_compressed takes.  The library keeps the proofs in flight itself; nothing is
     decoded or compressed on the host. *)
  let prove_many_compressed (qap : qap) (pkey : pkey) (sol : f Var.Map.t) (jobs : (Fr.t * Fr.t) list) : bytes list =
    let handle = handle_of qap pkey in
    if not (Var.Set.equal (Var.Map.domain sol) (Var.Map.domain qap.v)) then assert false;
    Mi355x.(check (zk_groth16_set_witness handle (bytes_start (fr_bytes (values sol)))));
    let rnd = Mi355x.cat (List.concat_map (fun (r, s) -> [ Fr.to_bytes r; Fr.to_bytes s ]) jobs) in
    Mi355x.prove_many_compressed Mi355x.zk_groth16_prove_many_compressed handle ~rnd ~count:(List.length jobs) ~size:192

  (* ---------------------------------------------------------------- check_key
     Is pkey a well-formed key of qap's circuit -- and, with ~vkey, the partner of that verification key?  Every relation of setup (groth16.ml:45-108)
     as one random combination on the device (zk_groth16_key_check); the names of the relations that do not hold, [] for a well-formed key.  vkey.ab is
     compared here, with the pairing of the key's own alpha and beta (groth16.ml:103), and reported as "ab": the library never sees it.  seed: 32 bytes
     drawn by the caller AFTER the key's bytes are fixed, from a cryptographic generator; without it the library draws them. *)
  let key_check_names ?(vkey : vkey option) (pkey : pkey) (mask : int) : string list =
    let names = List.filter_map (fun (bit, name) -> if mask land bit <> 0 then Some name else None) Mi355x.keychk_names in
    match vkey with
    | Some v when not GT.(Pairing.pairing pkey.a pkey.b2 = v.ab) -> names @ [ "ab" ]
    | _ -> names

  let vk_bytes (vkey : vkey option) = Option.map (fun (v : vkey) -> (g1_bytes (v.one1 :: values v.ltgm_io), g2_bytes [ v.one2; v.gm; v.d ])) vkey

  let check_key ?(vkey : vkey option) ?(seed : bytes option) (qap : qap) (pkey : pkey) : string list =
    let vk = vk_bytes vkey in
    key_check_names ?vkey pkey (Mi355x.groth16_key_check ?vk ?seed (handle_of qap pkey))

  (* The same for the key as the handle holds it in LAGRANGE form (zk_groth16_key_check_lagrange): after derive_lagrange_on_upload, or for `handle`
     from upload_compressed ~lagrange:true -- pools read back from a key cache, bytes from somewhere else until this has looked at them.  No derivation
     runs.  pkey gives alpha and beta for "ab"; the names are check_key's. *)
  let check_key_lagrange ?(vkey : vkey option) ?(seed : bytes option) ?(handle : Unsigned.UInt64.t option) (qap : qap) (pkey : pkey) : string list =
    let h = match handle with Some h -> h | None -> handle_of qap pkey in
    let vk = vk_bytes vkey in
    key_check_names ?vkey pkey (Mi355x.groth16_key_check_lagrange ?vk ?seed h)

  (* ---------------------------------------------------------------- contribute
     A phase-2 contribution on the device (zk_groth16_pk_contribute): delta <- delta dmul for the key the handle of (qap, pkey) holds -- d1, d2 times
     dmul, tiztd (or hl) and ltd_mid times 1 / dmul, new window tables, no host round trip.  Returns (d1 before | d1 after, [dmul]_2, d2 after), uncompressed:
     the link between the two keys and the d of the new verification key (ab and ltgm_io stay).  From here on the handle holds the CONTRIBUTED key, not
     pkey: proofs come out under it, and its bytes are read back through the pool calls (Mi355x.pool_points_compressed). *)
  let contribute (qap : qap) (pkey : pkey) ~(dmul : Fr.t) : bytes * bytes * bytes =
    Mi355x.groth16_pk_contribute (handle_of qap pkey) ~dmul:(Fr.to_bytes dmul)

  (* ---------------------------------------------------------------- verify
     e(A, B) = ab + e(sum_k w_k [L_k(tau)/gamma]_1, gamma) + e(C, delta), GT written additively as Curve.G has it.  The sum
     runs over the public coefficients; domains must agree (G.dot). *)
  let verify (input_output : f Var.Map.t) (vkey : vkey) (proof : proof) : bool =
    let e = Pairing.pairing in
    let public_part = G1.dot vkey.ltgm_io input_output in
    GT.(e proof.a proof.b - e public_part vkey.gm - e proof.c vkey.d = vkey.ab)

  (* ---------------------------------------------------------------- verify_many
     `verify` for a list of (public inputs, proof) under one key in ONE library call, on the device (zk_groth16_verify_many): the three
     pairings of every proof side by side.  A lone proof is quicker through `verify`.
     The library compares GT elements as the 12 Fp coefficients of the tower Fp12 = Fp6[w] / (w^2 - v), Fp6 = Fp2[v] / (v^3 - (1 + u)), 48 bytes
     big-endian each (include/zkmi355x.h); GT.to_bytes of opam bls12-381 writes the same coefficients in the same order, little-endian.  That is
     CHECKED, not assumed: before the first batch of a process e(G1.one, G2.one) is computed by both sides, and a difference fails before any proof
     is judged.  After that a batch is ONE library call. *)
  let gt_lib_bytes (x : GT.t) : bytes =
    let b = GT.to_bytes x in
    if Bytes.length b <> 576 then failwith "verify_many: GT.to_bytes is not 12 x 48 bytes";
    Bytes.init 576 (fun i -> Bytes.get b ((i / 48 * 48) + 47 - (i mod 48)))

  (* the check of that byte order: ONCE per process, at the first batch (a pairing on each side) *)
  let gt_order_checked =
    lazy
      (let probe = Bytes.create 576 in
       Mi355x.(
         check
           (zk_pairing_product
              (bytes_start (G1.to_bytes G1.one))
              (bytes_start (G2.to_bytes G2.one))
              (sz 1) (bytes_start probe)));
       if not (Bytes.equal probe (gt_lib_bytes (Pairing.pairing G1.one G2.one))) then
         failwith "verify_many: the library's GT encoding is not GT.to_bytes with every coefficient reversed")

  let verify_many (jobs : (f Var.Map.t * proof) list) (vkey : vkey) : bool list =
    List.iter (fun (io, _) -> assert (Var.Set.equal (Var.Map.domain io) (Var.Map.domain vkey.ltgm_io))) jobs;
    Lazy.force gt_order_checked;
    let count = List.length jobs in
    let ok = Bytes.make (max count 1) (Char.chr 0) in
    let io_all = fr_bytes (List.concat_map (fun (io, _) -> values io) jobs) in
    let proofs = Mi355x.cat (List.concat_map (fun (_, (p : proof)) -> [ G1.to_bytes p.a; G2.to_bytes p.b; G1.to_bytes p.c ]) jobs) in
    Mi355x.(
      check
        (zk_groth16_verify_many
           (bytes_start (gt_lib_bytes vkey.ab))
           (bytes_start (g1_bytes (values vkey.ltgm_io)))
           (sz (Var.Map.cardinal vkey.ltgm_io))
           (bytes_start (G2.to_bytes vkey.gm))
           (bytes_start (G2.to_bytes vkey.d))
           (bytes_start io_all) (bytes_start proofs) (u32 count) (bytes_start ok) no_status));
    List.init count (fun i -> Bytes.get ok i <> Char.chr 0)

  (* ---------------------------------------------------------------- Verifier
     The same for a STREAM of batches under one key: `create` hands the key to the device once (zk_groth16_vk_upload: its points decoded and
     checked there, a bad key point raises as in `verify`), every `verify_many` then moves only the proofs and their public inputs
     (zk_groth16_verify_resident), `free` releases the handle.  The lists are those of the function above on the same key. *)
  module Verifier = struct
    type t = { handle : Unsigned.UInt64.t; domain : Var.Set.t }

    let create (vkey : vkey) : t =
      Lazy.force gt_order_checked;
      let h = Ctypes.allocate Ctypes.uint64_t Unsigned.UInt64.zero in
      Mi355x.(
        check
          (zk_groth16_vk_upload
             (bytes_start (gt_lib_bytes vkey.ab))
             (bytes_start (g1_bytes (values vkey.ltgm_io)))
             (sz (Var.Map.cardinal vkey.ltgm_io))
             (bytes_start (G2.to_bytes vkey.gm))
             (bytes_start (G2.to_bytes vkey.d))
             h));
      { handle = Ctypes.( !@ ) h; domain = Var.Map.domain vkey.ltgm_io }

    let verify_many (t : t) (jobs : (f Var.Map.t * proof) list) : bool list =
      List.iter (fun (io, _) -> assert (Var.Set.equal (Var.Map.domain io) t.domain)) jobs;
      let count = List.length jobs in
      let ok = Bytes.make (max count 1) (Char.chr 0) in
      let io_all = fr_bytes (List.concat_map (fun (io, _) -> values io) jobs) in
      let proofs = Mi355x.cat (List.concat_map (fun (_, (p : proof)) -> [ G1.to_bytes p.a; G2.to_bytes p.b; G1.to_bytes p.c ]) jobs) in
      Mi355x.(check (zk_groth16_verify_resident t.handle (bytes_start io_all) (bytes_start proofs) (u32 count) (bytes_start ok) no_status));
      List.init count (fun i -> Bytes.get ok i <> Char.chr 0)

    (* Are ALL of these proofs good?  One folded pairing equation for the list (zk_groth16_verify_folded) instead of one per proof: the loop of
       test.ml:107-179 as one question.  The coefficients are drawn HERE, from `rng`, after the proofs are in hand: 16 bytes per proof, the low half of
       an Fr.gen (uniform up to 2^-127), a zero drawn again.  `rng` must be unpredictable to whoever made the proofs -- a seeded test generator is
       not; with known coefficients a bad list can be made to pass.  false: some proof is bad, and verify_many says which. *)
    let verify_all rng (t : t) (jobs : (f Var.Map.t * proof) list) : bool =
      List.iter (fun (io, _) -> assert (Var.Set.equal (Var.Map.domain io) t.domain)) jobs;
      let count = List.length jobs in
      let rec draw () =
        let b = Bytes.sub (Fr.to_bytes (Fr.gen rng)) 0 16 in
        if Bytes.equal b (Bytes.make 16 (Char.chr 0)) then draw () else b
      in
      let rho = Mi355x.cat (List.init count (fun _ -> draw ())) in
      let io_all = fr_bytes (List.concat_map (fun (io, _) -> values io) jobs) in
      let proofs = Mi355x.cat (List.concat_map (fun (_, (p : proof)) -> [ G1.to_bytes p.a; G2.to_bytes p.b; G1.to_bytes p.c ]) jobs) in
      let all_ok = Ctypes.allocate Ctypes.int 0 in
      Mi355x.(
        check (zk_groth16_verify_folded t.handle (bytes_start io_all) (bytes_start proofs) (bytes_start rho) (u32 count) all_ok no_status));
      Ctypes.( !@ ) all_ok <> 0

    (* The same two questions about proofs still in their wire form: each proof as the 192 bytes a | b | c
       of its record's fields under to_compressed_bytes -- what the proof's JSON holds, before of_compressed_bytes_exn.  The points are decompressed and
       checked on the device in the same call; a proof with a point that does not decode is false, as a proof that of_compressed_bytes_exn refuses
       never reaches verify. *)
    let compressed_jobs (t : t) (jobs : (f Var.Map.t * bytes) list) =
      List.iter
        (fun (io, p) ->
          assert (Var.Set.equal (Var.Map.domain io) t.domain);
          assert (Bytes.length p = 192))
        jobs;
      (fr_bytes (List.concat_map (fun (io, _) -> values io) jobs), Mi355x.cat (List.map snd jobs))

    let verify_many_compressed (t : t) (jobs : (f Var.Map.t * bytes) list) : bool list =
      let io_all, proofs = compressed_jobs t jobs in
      let count = List.length jobs in
      let ok = Bytes.make (max count 1) (Char.chr 0) in
      Mi355x.(
        check (zk_groth16_verify_resident_compressed t.handle (bytes_start io_all) (bytes_start proofs) (u32 count) (bytes_start ok) no_status));
      List.init count (fun i -> Bytes.get ok i <> Char.chr 0)

    let verify_all_compressed rng (t : t) (jobs : (f Var.Map.t * bytes) list) : bool =
      let io_all, proofs = compressed_jobs t jobs in
      let count = List.length jobs in
      let rec draw () =
        let b = Bytes.sub (Fr.to_bytes (Fr.gen rng)) 0 16 in
        if Bytes.equal b (Bytes.make 16 (Char.chr 0)) then draw () else b
      in
      let rho = Mi355x.cat (List.init count (fun _ -> draw ())) in
      let all_ok = Ctypes.allocate Ctypes.int 0 in
      Mi355x.(
        check
          (zk_groth16_verify_folded_compressed t.handle (bytes_start io_all) (bytes_start proofs) (bytes_start rho) (u32 count) all_ok no_status));
      Ctypes.( !@ ) all_ok <> 0

    let free (t : t) = Mi355x.vk_free t.handle
  end
end
