"""The folded Pinocchio equation itself (include/zkmi355x.h: zk_pinocchio_verify_folded), decided with big integers and pyref's pairing, no device:
tests/pinocchio_fold_model.py builds the count + 9 pairs from the oracle's key and two oracle proofs of iterated_cubic(2, x), x = 9, 10.  A good batch
is accepted, a wrong h is refused, and the two cancellations the header warns of -- across two proofs, and inside one -- pass under equal coefficients
and fail under different ones: the second is why a proof has five coefficients.  Each product of 11 pairings takes some seconds here; a test takes at
most two."""
import pytest

from oracle import pyref as P
from zukelang_amd import r1cs as RC
import oracle_lib as O
import pinocchio_fold_model as M

R = P.R
frs = lambda xs: b"".join(P.fr_to_bytes(x) for x in xs)
D = P.pt_mul(P.G1, 0xD15EA5E)


def rows(seed, n):
    st = P.fr_stream(seed)
    return [[(next(st) & ((1 << 128) - 1)) or 1 for _ in range(5)] for _ in range(n)]


@pytest.fixture(scope="module")
def batch():
    cs, _ = RC.iterated_cubic(2, 9)
    csr = [O.CSR(m.ptr, m.col, m.val) for m in (cs.L, cs.R, cs.O)]
    st = P.fr_stream(0x5EED0200)
    toxic = frs([next(st) for _ in range(8)])
    ex = O.pinocchio_keygen_exponents(None, cs.n, cs.m, *csr, cs.mid, toxic, False)
    vk1, vk2 = O.points_of_exponents_g1(ex[2]), O.points_of_exponents_g2(ex[3])
    ios, proofs = [], []
    for x in (9, 10):
        _, w = RC.iterated_cubic(2, x)
        dv, dw, dy = (P.fr_to_bytes(next(st)) for _ in range(3))
        proofs.append(O.pinocchio_prove_trapdoor(cs.n, cs.m, *csr, cs.mid, frs(w), toxic, dv, dw, dy))
        ios.append([w[k] for k in range(cs.m) if not cs.mid[k]])
    return vk1, vk2, ios, proofs


def holds(batch, proofs, rho):
    vk1, vk2, ios, _ = batch
    return P.pairing_product_is_one(M.fold(vk1, vk2, ios[:len(proofs)], proofs, rho)[2])


def test_a_good_batch_is_accepted_and_a_tripled_h_is_refused(batch):
    proofs = batch[3]
    rho = rows(0x5EED0201, 2)
    assert holds(batch, proofs, rho)
    h3 = M.moved(proofs[1], h=P.pt_mul(M.proof_points(proofs[1])["h"], 2))
    assert not holds(batch, [proofs[0], h3], rho)


def test_across_proofs_vavv_moved_by_d_and_minus_d_cancels_under_equal_coefficients(batch):
    proofs = batch[3]
    crafted = [M.moved(proofs[0], vavv=D), M.moved(proofs[1], vavv=P.pt_neg(D))]
    rho = rows(0x5EED0202, 2)
    assert not holds(batch, crafted, rho)
    rho[1][0] = rho[0][0]                                                # rho_00 = rho_10
    assert holds(batch, crafted, rho)


def test_inside_one_proof_vavv_and_yayy_cancel_at_one2_under_equal_coefficients(batch):
    proofs = batch[3]
    crafted = [M.moved(proofs[0], vavv=D, yayy=P.pt_neg(D))]
    rho = rows(0x5EED0203, 1)
    assert not holds(batch, crafted, rho)
    rho[0][2] = rho[0][0]                                                # rho_i0 = rho_i2: one coefficient per proof would always be this case
    assert holds(batch, crafted, rho)
