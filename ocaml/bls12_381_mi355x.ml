(* bls12_381_mi355x.ml -- seam 1: a GPU-backed instance of Curve.S (src/lib/zk/curve.mli:46-54).

   Goes to src/lib/zk/.  `Groth16.Make(Bls12_381_mi355x)` / `Pinocchio.Make(Bls12_381_mi355x)` then run the reference's
   protocol code UNCHANGED with every `apply_powers`, `dot` and `powers` (curve.ml:91-118) executed as one multi-scalar
   product / fixed-base kernel on the MI355X.  The O(m n) structure of `sum_apply_powers` (groth16.ml:116-121) remains with
   this seam alone -- seam 2 (groth16_mi355x.ml, pinocchio_mi355x.ml) removes it.

   Fr, GT and Pairing are the host's own (opam bls12-381): the verifier of ONE proof needs a handful of pairings, not a GPU.  Lists of
   proofs are checked on the device by `verify_many` of the seam-2 modules (groth16_mi355x.ml, pinocchio_mi355x.ml). *)

module Base = Curve.Bls12_381

module Make_group (G : sig
  include Curve.G with type fr := Base.Fr.t

  val to_bytes : t -> bytes
  val of_bytes_exn : bytes -> t
  val g2 : bool
  val point_bytes : int
end) =
struct
  include G

  let scalars_bytes (cs : Base.Fr.t list) = Mi355x.cat (List.map Bls12_381.Fr.to_bytes cs)
  let points_bytes (ps : t list) = Mi355x.cat (List.map to_bytes ps)

  let split (b : bytes) : t list =
    List.init (Bytes.length b / point_bytes) (fun i -> of_bytes_exn (Bytes.sub b (point_bytes * i) point_bytes))

  (* G.of_Fr over a list: one fixed-base launch (curve.ml:180 mapped) *)
  let of_Fr_many (ss : Base.Fr.t list) : t list = split (Mi355x.of_fr_many ~g2 (scalars_bytes ss))

  (* curve.ml:106-109: d + 1 points g^(s^0) .. g^(s^d) *)
  let powers d s = split (Mi355x.powers ~g2 d (Bls12_381.Fr.to_bytes s))

  (* Resident bases (header, "resident MSM bases").  apply_powers memoises a device handle on the PHYSICAL xis list, dot on the physical key
     map m (never on the fresh list Var.Map.bindings builds): the reference multiplies the same list again and again (sum_apply_powers,
     groth16.ml:116-121; dot on the key maps of every proof, curve.ml:94-103).  The first call on a list goes through zk_msm_* as before, the
     second uploads it, every later one multiplies the resident copy.  Ephemeron tables: an entry dies with its key, whose finaliser frees
     the handle.  The hash is Hashtbl.hash, which looks at a bounded number of words whatever the list's length (List.length is O(n)). *)
  type memo = Seen | Resident of Unsigned.UInt64.t | Refused

  module By_list = Ephemeron.K1.Make (struct
    type nonrec t = t list

    let equal = ( == )
    let hash (k : t) = Hashtbl.hash k
  end)

  module By_map = Ephemeron.K1.Make (struct
    type nonrec t = t Var.Map.t

    let equal = ( == )
    let hash (k : t) = Hashtbl.hash k
  end)

  let by_list : memo By_list.t = By_list.create 16
  let by_map : memo By_map.t = By_map.create 16

  (* sum_i c_i x_i over the first (length cs) points of a resident list *)
  let resident_apply h (cs : Base.Fr.t list) : t =
    let sc = scalars_bytes cs and out = Bytes.create point_bytes in
    Mi355x.(check (zk_msm_resident h (bytes_start sc) (sz (Bytes.length sc / 32)) (bytes_start out)));
    of_bytes_exn out

  (* the handle of `key` if it has one, uploading on the second sight; None: go through zk_msm_* (first sight, or the upload failed) *)
  let resident ~find ~replace key (points : unit -> bytes) =
    match find key with
    | Some (Resident h) -> Some h
    | Some Refused -> None
    | None ->
        replace key Seen;
        None
    | Some Seen -> (
        match Mi355x.resident_upload ~g2 (points ()) with
        | h ->
            (try Gc.finalise (fun _ -> Mi355x.resident_free h) key with Invalid_argument _ -> ());
            replace key (Resident h);
            Some h
        | exception _ ->
            replace key Refused;
            None)

  (* curve.ml:112-118: sum_i c_i x_i; runs out of coefficients quietly, of points with Invalid_argument "apply_powers" *)
  let apply_powers (cs : Base.Fr.t Polynomial.t) (xis : t list) : t =
    match cs, xis with
    | [], _ -> zero
    | _, [] -> of_bytes_exn (Mi355x.msm ~g2 (points_bytes xis) (scalars_bytes cs))
    | _ -> (
        match resident ~find:(By_list.find_opt by_list) ~replace:(By_list.replace by_list) xis (fun () -> points_bytes xis) with
        | Some h -> resident_apply h cs
        | None -> of_bytes_exn (Mi355x.msm ~g2 (points_bytes xis) (scalars_bytes cs)))

  (* curve.ml:94-103: equal key sets or `assert false` *)
  let dot (m : t Var.Map.t) (c : Base.Fr.t Var.Map.t) : t =
    if not (Var.Set.equal (Var.Map.domain m) (Var.Map.domain c)) then assert false;
    match List.map snd (Var.Map.bindings c) with
    | [] -> zero
    | cs -> (
        let points () = points_bytes (List.map snd (Var.Map.bindings m)) in
        match resident ~find:(By_map.find_opt by_map) ~replace:(By_map.replace by_map) m points with
        | Some h -> resident_apply h cs
        | None -> of_bytes_exn (Mi355x.msm ~g2 (points ()) (scalars_bytes cs)))
end

module Fr = Base.Fr
module GT = Base.GT
module Pairing = Base.Pairing

(* Curve.Bls12_381 is sealed to Curve.S, which has no byte access; the type equalities it exports (curve.mli:56-60) let the
   opam module's own to_bytes / of_bytes_exn be used on its points. *)
module G1 = Make_group (struct
  include Base.G1

  let to_bytes = Bls12_381.G1.to_bytes
  let of_bytes_exn = Bls12_381.G1.of_bytes_exn
  let g2 = false
  let point_bytes = 96
end)

module G2 = Make_group (struct
  include Base.G2

  let to_bytes = Bls12_381.G2.to_bytes
  let of_bytes_exn = Bls12_381.G2.of_bytes_exn
  let g2 = true
  let point_bytes = 192
end)
