(* pinocchio_mi355x.ml -- seam 2 for Pinocchio Protocol 2: the body of src/pinocchio/pinocchio.ml with the prover on the MI355X.

   Install as src/pinocchio/pinocchio.ml; pinocchio.mli stays byte-identical (Make(C).NonZK / ZK : Protocol.S).  Needs the two
   `val`s in `Curve.G` described in groth16_mi355x.ml.

   What is replaced (reference lines):
     ZK.prove     pinocchio.ml:559-561 + ZKCompute.f :427-514 + QAP.eval  -> zk_pinocchio_prove; dv, dw, dy drawn HERE in the
                  order of :428-430
     NonZK.prove  pinocchio.ml:536-538 + Compute.f :210-248                -> the same call with dv = dw = dy = 0 (no rng use)
     keygen       pinocchio.ml:530-534 + KeyGen.generate :77-189           -> one call zk_pinocchio_keygen (rv, rw, s, av, aw, ay, b, gm drawn
                  HERE in the order of :83-91; exponents and points are the device's; a multi-device list: the bytes, then the ordinary upload)
     verify       pinocchio.ml:540-541,563 + Verify.f :254-420             -> zk_pinocchio_verify (13 pairings on the host, in the
                  library: it takes only G1 / G2 points, so no GT encoding is involved).  Where the reference `assert`s the
                  four knowledge-of-coefficient checks and returns the divisibility check, this returns false for any failing
                  check.
     verify_many  (an extra) a list of proofs under one key              -> one call zk_pinocchio_verify_many, the pairings on the device
     Verifier     (an extra) the key resident on the device: create / verify_many / free -> a call moves only proofs and public inputs
   Records and their yojson are the reference's (pinocchio.ml:37-75,195-208). *)

open Zukelang
open Yojson_conv

module Make (C : Curve.S) = struct
  open C
  module Circuit = Circuit.Make (C.Fr)
  module QAP = QAP.Make (C.Fr)
  module Poly = QAP.Polynomial

  type circuit = Circuit.t
  type qap = QAP.t

  type pkey =
    { vv : G1.t Var.Map.t;
      ww : G2.t Var.Map.t;
      yy : G1.t Var.Map.t;
      vav : G1.t Var.Map.t;
      waw : G2.t Var.Map.t;
      yay : G1.t Var.Map.t;
      si : G1.t list;
      bvwy : G1.t Var.Map.t;
      si2 : G2.t list;
      vt : G1.t;
      wt : G2.t;
      yt : G1.t;
      vavt : G1.t;
      wawt : G2.t;
      yayt : G1.t;
      vbt : G1.t;
      wbt : G1.t;
      ybt : G1.t;
      v_all : G1.t Var.Map.t;
      w_all : G1.t Var.Map.t
    }
  [@@deriving yojson]

  type vkey =
    { one : G1.t;
      one2 : G2.t;
      av : G2.t;
      aw : G1.t;
      ay : G2.t;
      gm2 : G2.t;
      bgm : G1.t;
      bgm2 : G2.t;
      yt : G2.t;
      vv_io : G1.t Var.Map.t;
      ww_io : G2.t Var.Map.t;
      yy_io : G1.t Var.Map.t
    }
  [@@deriving yojson]

  type proof =
    { vv : G1.t;
      ww : G2.t;
      yy : G1.t;
      h : G1.t;
      vavv : G1.t;
      waww : G2.t;
      yayy : G1.t;
      bvwy : G1.t
    }
  [@@deriving yojson]

  let fr_bytes (xs : Fr.t list) = Mi355x.cat (List.map Fr.to_bytes xs)
  let g1_bytes (ps : G1.t list) = Mi355x.cat (List.map G1.to_bytes ps)
  let g2_bytes (ps : G2.t list) = Mi355x.cat (List.map G2.to_bytes ps)
  let g1_at b i = G1.of_bytes_exn (Bytes.sub b (96 * i) 96)
  let g2_at b i = G2.of_bytes_exn (Bytes.sub b (192 * i) 192)
  let values m = List.map snd (Var.Map.bindings m)
  let keys m = List.map fst (Var.Map.bindings m)

  (* ---------------------------------------------------------------- circuit rows (as in groth16_mi355x.ml) *)

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
    (Mi355x.matrix_of_rows (rows qap.QAP.v), Mi355x.matrix_of_rows (rows qap.QAP.w), Mi355x.matrix_of_rows (rows qap.QAP.y))

  (* ---------------------------------------------------------------- uploaded keys: pools in the order of include/zkmi355x.h
       g1: vv | yy | vav | yay | bvwy (I_mid each) | si (n+1) | v_all (m) | w_all (m) | vt | yt | vavt | yayt | vbt | wbt | ybt
       g2: ww | waw (I_mid each) | si2 (n+1) | wt | wawt *)

  module Handles = Ephemeron.K1.Make (struct
    type t = pkey

    let equal = ( == )
    let hash (k : pkey) = List.length k.si
  end)

  let handles : Unsigned.UInt64.t Handles.t = Handles.create 8
  let derive_lagrange_on_upload = ref false

  let upload (vars : Var.t list) (l, r, o) n (k : pkey) : Unsigned.UInt64.t =
    let var_at = Array.of_list vars in
    let m = Array.length var_at in
    let mid = Bytes.init m (fun i -> if Var.Map.mem var_at.(i) k.vv then '\001' else '\000') in
    let g1 =
      g1_bytes
        (values k.vv @ values k.yy @ values k.vav @ values k.yay @ values k.bvwy @ k.si @ values k.v_all @ values k.w_all
        @ [ k.vt; k.yt; k.vavt; k.yayt; k.vbt; k.wbt; k.ybt ])
    in
    let g2 = g2_bytes (values k.ww @ values k.waw @ k.si2 @ [ k.wt; k.wawt ]) in
    let h = Mi355x.pinocchio_upload ~n ~m l r o ~mid ~g1 ~g2 in
    if !derive_lagrange_on_upload then Mi355x.(check (zk_pinocchio_pk_derive_lagrange h));
    Gc.finalise (fun _ -> ignore (Mi355x.zk_pinocchio_pk_free h)) k;
    Handles.replace handles k h;
    h

  (* a key whose bytes exist on the host -- read from JSON, or generated while the device list had several entries -- enters the library here *)
  let register = upload

  (* The same from the record's COMPRESSED strings as they stand in the JSON (zk_pinocchio_pk_upload_compressed), in the pool order above, 48 / 96 B per
     point, decoded and checked on the device.  h_lagrange: the n stored h bases of a derived key (the first n points of pool 5 in wire form).  The
     handle is registered under the key like any other. *)
  let upload_compressed ?h_lagrange (vars : Var.t list) (l, r, o) n (k : pkey) ~(g1 : bytes) ~(g2 : bytes) : Unsigned.UInt64.t =
    let var_at = Array.of_list vars in
    let m = Array.length var_at in
    let mid = Bytes.init m (fun i -> if Var.Map.mem var_at.(i) k.vv then '\001' else '\000') in
    let h = Mi355x.pinocchio_upload_compressed ?h_lagrange ~n ~m l r o ~mid ~g1 ~g2 in
    Gc.finalise (fun _ -> ignore (Mi355x.zk_pinocchio_pk_free h)) k;
    Handles.replace handles k h;
    h

  let pool_compressed (h : Unsigned.UInt64.t) ~(pool : int) : bytes =
    Mi355x.pool_points_compressed Mi355x.zk_pinocchio_pool_points_compressed h ~pool ~point_bytes:(if pool < 6 then 48 else 96)

  let handle_of (qap : qap) (k : pkey) =
    match Handles.find_opt handles k with
    | Some h -> h
    | None ->
        let vars = keys qap.QAP.v in
        let n = Poly.degree qap.QAP.target in
        upload vars (matrices_of_qap (index_of_vars vars) qap n) n k

  (* ---------------------------------------------------------------- keygen *)

  let keygen rng (circuit : circuit) (qap : qap) : pkey * vkey =
    let n = Poly.degree qap.QAP.target in
    let rv = Fr.gen rng in
    let rw = Fr.gen rng in
    let s = Fr.gen rng in
    let av = Fr.gen rng in
    let aw = Fr.gen rng in
    let ay = Fr.gen rng in
    let b = Fr.gen rng in
    let gm = Fr.gen rng in
    (* ONE library call (zk_pinocchio_keygen): the exponents of pinocchio.ml:93-175 on the device, the points by the fixed-base kernel; the
       bytes are the evaluation and verification keys in the reference's format, the handle already holds the derived h pool (a device list of
       one entry; on a longer list no handle is offered and the bytes are registered like a key read from JSON, below). *)
    let vars = keys qap.QAP.v in
    let m = List.length vars in
    let mids = circuit.Circuit.mids and ios = Circuit.ios circuit in
    let n_mid = Var.Set.cardinal mids and n_io = Var.Set.cardinal ios in
    if n_mid + n_io <> m then assert false;
    let mid = Mi355x.cat (List.map (fun v -> Bytes.make 1 (if Var.Set.mem v mids then '\001' else '\000')) vars) in
    let l, r, o = matrices_of_gates (index_of_vars vars) circuit.Circuit.gates in
    let p1, p2, v1, v2, h =
      Mi355x.keygen_call Mi355x.zk_pinocchio_keygen ~n ~m l r o ~mid
        ~toxic:(fr_bytes [ rv; rw; s; av; aw; ay; b; gm ])
        ~form:Mi355x.key_form_lagrange
        ~g1_points:((5 * n_mid) + n + 1 + (2 * m) + 7)
        ~g2_points:((2 * n_mid) + n + 1 + 2)
        ~vk1_points:(3 + (2 * n_io))
        ~vk2_points:(6 + n_io)
    in
    let map_of set at buf off = Var.Map.of_list (List.mapi (fun i k -> (k, at buf (off + i))) (Var.Set.elements set)) in
    let all_vars = Var.Set.of_list vars in
    let o_si = 5 * n_mid in
    let o_all = o_si + n + 1 in
    let o_single = o_all + (2 * m) in
    let o2_si = 2 * n_mid in
    let o2_single = o2_si + n + 1 in
    let pkey : pkey =
      { vv = map_of mids g1_at p1 0;
        yy = map_of mids g1_at p1 n_mid;
        vav = map_of mids g1_at p1 (2 * n_mid);
        yay = map_of mids g1_at p1 (3 * n_mid);
        bvwy = map_of mids g1_at p1 (4 * n_mid);
        si = List.init (n + 1) (fun i -> g1_at p1 (o_si + i));
        v_all = map_of all_vars g1_at p1 o_all;
        w_all = map_of all_vars g1_at p1 (o_all + m);
        vt = g1_at p1 o_single;
        yt = g1_at p1 (o_single + 1);
        vavt = g1_at p1 (o_single + 2);
        yayt = g1_at p1 (o_single + 3);
        vbt = g1_at p1 (o_single + 4);
        wbt = g1_at p1 (o_single + 5);
        ybt = g1_at p1 (o_single + 6);
        ww = map_of mids g2_at p2 0;
        waw = map_of mids g2_at p2 n_mid;
        si2 = List.init (n + 1) (fun i -> g2_at p2 (o2_si + i));
        wt = g2_at p2 o2_single;
        wawt = g2_at p2 (o2_single + 1)
      }
    in
    let vkey : vkey =
      { one = g1_at v1 0;
        one2 = g2_at v2 0;
        aw = g1_at v1 1;
        bgm = g1_at v1 2;
        vv_io = map_of ios g1_at v1 3;
        yy_io = map_of ios g1_at v1 (3 + n_io);
        av = g2_at v2 1;
        ay = g2_at v2 2;
        gm2 = g2_at v2 3;
        bgm2 = g2_at v2 4;
        yt = g2_at v2 5;
        ww_io = map_of ios g2_at v2 6
      }
    in
    (match h with
    | Some h ->
        Gc.finalise (fun _ -> ignore (Mi355x.zk_pinocchio_pk_free h)) pkey;
        Handles.replace handles pkey h
    | None ->
        (* a device list of several entries (Mi355x.use_all_devices): the generated bytes go through zk_pinocchio_pk_upload, which cuts every pool over
           the list behind one handle; derive_lagrange_on_upload applies to it as to any uploaded key *)
        ignore (register vars (l, r, o) n pkey));
    (pkey, vkey)

  (* ---------------------------------------------------------------- prove *)

  let prove_with (qap : qap) (k : pkey) (sol : Fr.t Var.Map.t) dv dw dy : proof =
    let handle = handle_of qap k in
    if not (Var.Set.equal (Var.Map.domain sol) (Var.Map.domain qap.QAP.v)) then assert false;
    let out = Bytes.create 960 in
    Mi355x.(
      check
        (zk_pinocchio_prove handle
           (bytes_start (fr_bytes (values sol)))
           (bytes_start (Fr.to_bytes dv))
           (bytes_start (Fr.to_bytes dw))
           (bytes_start (Fr.to_bytes dy))
           (bytes_start out)));
    (* Compute.proof, pinocchio.ml:195-208: vv | ww (G2) | yy | h | vavv | waww (G2) | yayy | bvwy *)
    let g1 off = G1.of_bytes_exn (Bytes.sub out off 96) and g2 off = G2.of_bytes_exn (Bytes.sub out off 192) in
    { vv = g1 0; ww = g2 96; yy = g1 288; h = g1 384; vavv = g1 480; waww = g2 576; yayy = g1 768; bvwy = g1 864 }

  (* A batch of proofs of one witness in ONE library call, each as its 480 wire bytes (zk_pinocchio_prove_many_compressed): the eight strings of the
     proof record (pinocchio.ml:195-208) back to back, what Resident.verify_many_compressed takes.  jobs: the (dv, dw, dy) of each proof in the order
     the reference draws them (:428-430); all zero is NonZK.  Nothing is decoded or compressed on the host. *)
  let prove_many_with (qap : qap) (k : pkey) (sol : Fr.t Var.Map.t) (jobs : (Fr.t * Fr.t * Fr.t) list) : bytes list =
    let handle = handle_of qap k in
    if not (Var.Set.equal (Var.Map.domain sol) (Var.Map.domain qap.QAP.v)) then assert false;
    Mi355x.(check (zk_pinocchio_set_witness handle (bytes_start (fr_bytes (values sol)))));
    let rnd = fr_bytes (List.concat_map (fun (dv, dw, dy) -> [ dv; dw; dy ]) jobs) in
    Mi355x.prove_many_compressed Mi355x.zk_pinocchio_prove_many_compressed handle ~rnd ~count:(List.length jobs) ~size:480

  let verify_with (ios : Fr.t Var.Map.t) (vk : vkey) (p : proof) : bool =
    (* the reference asserts equal domains before each of its three sums (pinocchio.ml:372,381,390) *)
    assert (Var.Set.equal (Var.Map.domain ios) (Var.Map.domain vk.vv_io));
    assert (Var.Set.equal (Var.Map.domain ios) (Var.Map.domain vk.ww_io));
    assert (Var.Set.equal (Var.Map.domain ios) (Var.Map.domain vk.yy_io));
    let vk_g1 = g1_bytes ((vk.one :: vk.aw :: vk.bgm :: values vk.vv_io) @ values vk.yy_io) in
    let vk_g2 = g2_bytes ((vk.one2 :: vk.av :: vk.ay :: vk.gm2 :: vk.bgm2 :: vk.yt :: values vk.ww_io)) in
    let proof_bytes =
      Mi355x.cat
        [ G1.to_bytes p.vv; G2.to_bytes p.ww; G1.to_bytes p.yy; G1.to_bytes p.h; G1.to_bytes p.vavv; G2.to_bytes p.waww;
          G1.to_bytes p.yayy; G1.to_bytes p.bvwy ]
    in
    let ok = Ctypes.allocate Ctypes.int 0 in
    Mi355x.(
      check
        (zk_pinocchio_verify (bytes_start vk_g1) (bytes_start vk_g2)
           (bytes_start (fr_bytes (values ios)))
           (sz (Var.Map.cardinal ios))
           (bytes_start proof_bytes) ok));
    Ctypes.( !@ ) ok <> 0

  (* verify_with for a list of (public inputs, proof) under one key in ONE library call, on the device (zk_pinocchio_verify_many): the 13 pairings
     of every proof side by side.  Only G1 / G2 points cross, as in verify_with.  A lone proof is quicker through verify_with. *)
  let verify_many_with (jobs : (Fr.t Var.Map.t * proof) list) (vk : vkey) : bool list =
    List.iter
      (fun (ios, _) ->
        assert (Var.Set.equal (Var.Map.domain ios) (Var.Map.domain vk.vv_io));
        assert (Var.Set.equal (Var.Map.domain ios) (Var.Map.domain vk.ww_io));
        assert (Var.Set.equal (Var.Map.domain ios) (Var.Map.domain vk.yy_io)))
      jobs;
    let vk_g1 = g1_bytes ((vk.one :: vk.aw :: vk.bgm :: values vk.vv_io) @ values vk.yy_io) in
    let vk_g2 = g2_bytes (vk.one2 :: vk.av :: vk.ay :: vk.gm2 :: vk.bgm2 :: vk.yt :: values vk.ww_io) in
    let proofs =
      Mi355x.cat
        (List.concat_map
           (fun (_, (p : proof)) ->
             [ G1.to_bytes p.vv; G2.to_bytes p.ww; G1.to_bytes p.yy; G1.to_bytes p.h; G1.to_bytes p.vavv; G2.to_bytes p.waww;
               G1.to_bytes p.yayy; G1.to_bytes p.bvwy ])
           jobs)
    in
    let count = List.length jobs in
    let ok = Bytes.make (max count 1) (Char.chr 0) in
    let io_all = fr_bytes (List.concat_map (fun (ios, _) -> values ios) jobs) in
    Mi355x.(
      check
        (zk_pinocchio_verify_many (bytes_start vk_g1) (bytes_start vk_g2)
           (sz (Var.Map.cardinal vk.vv_io))
           (bytes_start io_all) (bytes_start proofs) (u32 count) (bytes_start ok) no_status));
    List.init count (fun i -> Bytes.get ok i <> Char.chr 0)

  (* The same for a STREAM of batches under one key: `create` hands the key to the device once (zk_pinocchio_vk_upload: its points decoded and checked
     there, a bad key point raises as in verify_with), every `verify_many` then moves only the proofs and their public inputs
     (zk_pinocchio_verify_resident), `free` releases the handle.  Serves NonZK and ZK alike: they share the verifier. *)
  module Verifier = struct
    type t = { handle : Unsigned.UInt64.t; domain : Var.Set.t }

    let create (vk : vkey) : t =
      assert (Var.Set.equal (Var.Map.domain vk.vv_io) (Var.Map.domain vk.ww_io));
      assert (Var.Set.equal (Var.Map.domain vk.vv_io) (Var.Map.domain vk.yy_io));
      let vk_g1 = g1_bytes ((vk.one :: vk.aw :: vk.bgm :: values vk.vv_io) @ values vk.yy_io) in
      let vk_g2 = g2_bytes (vk.one2 :: vk.av :: vk.ay :: vk.gm2 :: vk.bgm2 :: vk.yt :: values vk.ww_io) in
      let h = Ctypes.allocate Ctypes.uint64_t Unsigned.UInt64.zero in
      Mi355x.(check (zk_pinocchio_vk_upload (bytes_start vk_g1) (bytes_start vk_g2) (sz (Var.Map.cardinal vk.vv_io)) h));
      { handle = Ctypes.( !@ ) h; domain = Var.Map.domain vk.vv_io }

    let verify_many (t : t) (jobs : (Fr.t Var.Map.t * proof) list) : bool list =
      List.iter (fun (ios, _) -> assert (Var.Set.equal (Var.Map.domain ios) t.domain)) jobs;
      let proofs =
        Mi355x.cat
          (List.concat_map
             (fun (_, (p : proof)) ->
               [ G1.to_bytes p.vv; G2.to_bytes p.ww; G1.to_bytes p.yy; G1.to_bytes p.h; G1.to_bytes p.vavv; G2.to_bytes p.waww;
                 G1.to_bytes p.yayy; G1.to_bytes p.bvwy ])
             jobs)
      in
      let count = List.length jobs in
      let ok = Bytes.make (max count 1) (Char.chr 0) in
      let io_all = fr_bytes (List.concat_map (fun (ios, _) -> values ios) jobs) in
      Mi355x.(check (zk_pinocchio_verify_resident t.handle (bytes_start io_all) (bytes_start proofs) (u32 count) (bytes_start ok) no_status));
      List.init count (fun i -> Bytes.get ok i <> Char.chr 0)

    (* Are ALL of these proofs good?  One folded pairing equation for the list (zk_pinocchio_verify_folded) instead of five per proof.  FIVE
       coefficients per proof, one per equation of Verify.f, are drawn HERE, from `rng`, after the proofs are in hand: 16 bytes each, the low half of
       an Fr.gen (uniform up to 2^-127), a zero drawn again.  `rng` must be unpredictable to whoever made the proofs -- a seeded test generator is
       not; with known coefficients a bad list, or one bad proof, can be made to pass.  false: some proof is bad, and verify_many says which. *)
    let verify_all rng (t : t) (jobs : (Fr.t Var.Map.t * proof) list) : bool =
      List.iter (fun (ios, _) -> assert (Var.Set.equal (Var.Map.domain ios) t.domain)) jobs;
      let count = List.length jobs in
      let rec draw () =
        let b = Bytes.sub (Fr.to_bytes (Fr.gen rng)) 0 16 in
        if Bytes.equal b (Bytes.make 16 (Char.chr 0)) then draw () else b
      in
      let rho = Mi355x.cat (List.init (5 * count) (fun _ -> draw ())) in
      let io_all = fr_bytes (List.concat_map (fun (ios, _) -> values ios) jobs) in
      let proofs =
        Mi355x.cat
          (List.concat_map
             (fun (_, (p : proof)) ->
               [ G1.to_bytes p.vv; G2.to_bytes p.ww; G1.to_bytes p.yy; G1.to_bytes p.h; G1.to_bytes p.vavv; G2.to_bytes p.waww;
                 G1.to_bytes p.yayy; G1.to_bytes p.bvwy ])
             jobs)
      in
      let all_ok = Ctypes.allocate Ctypes.int 0 in
      Mi355x.(
        check (zk_pinocchio_verify_folded t.handle (bytes_start io_all) (bytes_start proofs) (bytes_start rho) (u32 count) all_ok no_status));
      Ctypes.( !@ ) all_ok <> 0

    (* The same two questions about proofs still in their wire form: each proof as the 480 bytes vv | ww | yy | h | vavv | waww | yayy | bvwy
       of its record's fields under to_compressed_bytes -- what the proof's JSON holds, before of_compressed_bytes_exn.  The points are decompressed and
       checked on the device in the same call; a proof with a point that does not decode is false, as a proof that of_compressed_bytes_exn refuses
       never reaches verify. *)
    let compressed_jobs (t : t) (jobs : (Fr.t Var.Map.t * bytes) list) =
      List.iter
        (fun (io, p) ->
          assert (Var.Set.equal (Var.Map.domain io) t.domain);
          assert (Bytes.length p = 480))
        jobs;
      (fr_bytes (List.concat_map (fun (io, _) -> values io) jobs), Mi355x.cat (List.map snd jobs))

    let verify_many_compressed (t : t) (jobs : (Fr.t Var.Map.t * bytes) list) : bool list =
      let io_all, proofs = compressed_jobs t jobs in
      let count = List.length jobs in
      let ok = Bytes.make (max count 1) (Char.chr 0) in
      Mi355x.(
        check (zk_pinocchio_verify_resident_compressed t.handle (bytes_start io_all) (bytes_start proofs) (u32 count) (bytes_start ok) no_status));
      List.init count (fun i -> Bytes.get ok i <> Char.chr 0)

    let verify_all_compressed rng (t : t) (jobs : (Fr.t Var.Map.t * bytes) list) : bool =
      let io_all, proofs = compressed_jobs t jobs in
      let count = List.length jobs in
      let rec draw () =
        let b = Bytes.sub (Fr.to_bytes (Fr.gen rng)) 0 16 in
        if Bytes.equal b (Bytes.make 16 (Char.chr 0)) then draw () else b
      in
      let rho = Mi355x.cat (List.init (5 * count) (fun _ -> draw ())) in
      let all_ok = Ctypes.allocate Ctypes.int 0 in
      Mi355x.(
        check
          (zk_pinocchio_verify_folded_compressed t.handle (bytes_start io_all) (bytes_start proofs) (bytes_start rho) (u32 count) all_ok no_status));
      Ctypes.( !@ ) all_ok <> 0

    let free (t : t) = Mi355x.vk_free t.handle
  end

  module NonZK = struct
    type f = C.Fr.t
    type nonrec circuit = circuit
    type nonrec qap = qap
    type nonrec pkey = pkey [@@deriving yojson]
    type nonrec vkey = vkey [@@deriving yojson]
    type nonrec proof = proof [@@deriving yojson]

    let keygen = keygen
    let prove _rng qap pkey sol = prove_with qap pkey sol Fr.zero Fr.zero Fr.zero
    let prove_many _rng qap pkey sol count = prove_many_with qap pkey sol (List.init count (fun _ -> (Fr.zero, Fr.zero, Fr.zero)))
    let verify input_output vkey proof = verify_with input_output vkey proof
    let verify_many jobs vkey = verify_many_with jobs vkey
  end

  module ZK = struct
    type f = C.Fr.t
    type nonrec circuit = circuit
    type nonrec qap = qap
    type nonrec pkey = pkey [@@deriving yojson]
    type nonrec vkey = vkey [@@deriving yojson]
    type nonrec proof = proof [@@deriving yojson]

    let keygen = keygen

    let prove rng qap pkey sol =
      let dv = Fr.gen rng in
      let dw = Fr.gen rng in
      let dy = Fr.gen rng in
      prove_with qap pkey sol dv dw dy

    (* `count` proofs of one witness, dv, dw, dy drawn per proof in proof order; the proofs' wire bytes *)
    let prove_many rng qap pkey sol count =
      let draw _ =
        let dv = Fr.gen rng in
        let dw = Fr.gen rng in
        let dy = Fr.gen rng in
        (dv, dw, dy)
      in
      let rec jobs i acc = if i = count then List.rev acc else jobs (i + 1) (draw i :: acc) in
      prove_many_with qap pkey sol (jobs 0 [])

    let verify = NonZK.verify
    let verify_many = NonZK.verify_many
  end
end
