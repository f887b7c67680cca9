"""CPU: the two references of tests/segments_cases.py agree -- pymodel.Curve.msm_naive term by term, and the discrete-log identity
sum s_i (h_i G) = ((sum s_i h_i) mod r) G -- on planted bases (infinities, equal and opposite neighbours), and both see a scalar that
moves to the neighbouring segment: the two neighbours change and nothing else does."""
import pytest

import pymodel as pm
import segments_cases as sc


@pytest.mark.parametrize("name", ["bls12_381_g1", "bls12_377_g2"])
def test_the_two_references_agree(name):
    curve = pm.CURVES[name]
    lengths = [0, 1, 2, 18, 0, 20]
    offsets = sc.offsets_of(lengths)
    n = offsets[-1]
    logs, pts, imgs = sc.base_set(name, "planted", n)
    assert len(imgs) == n * curve.affine_stride and pts[1] is None
    assert any(p is None for p in pts) and any(pts[i] is not None and pts[i] == pts[i - 1] for i in range(1, n))
    assert any(pts[i] is not None and pts[i - 1] is not None and pts[i] == curve.neg(pts[i - 1]) for i in range(1, n))
    scalars = (sc.edge_scalars(curve) + sc.random_scalars(n, 0x2EF))[:n]
    naive = sc.expected_naive(curve, pts, scalars, offsets)
    dlog = sc.expected_dlog(curve, logs, scalars, offsets)
    assert naive == dlog
    assert naive[0] is None and naive[4] is None
    # one pair moves from segment 3 to segment 5 (segment 4 is empty: the boundary pair of 3 becomes the first of 5)
    moved = list(offsets)
    moved[4] -= 1
    moved[5] -= 1
    for ref in (sc.expected_naive(curve, pts, scalars, moved), sc.expected_dlog(curve, logs, scalars, moved)):
        changed = [s for s in range(len(lengths)) if ref[s] != naive[s]]
        assert changed == [3, 5], changed


def test_images_and_extremes():
    curve = pm.BLS12_381_G1
    assert sc.images(curve, [None]) == bytes(96) + b"\x01" + bytes(7)
    assert len(sc.images(curve, [None, curve.generator()], projective=True, stride=152)) == 304
    for c in range(2, 10):
        for s in sc.alternating_extremes(c):
            d = sc.booth_digits(s, c)
            assert sum(x << (c * j) for j, x in enumerate(d)) == s and max(d) == 1 << (c - 1) and min(d) == -(1 << (c - 1))
