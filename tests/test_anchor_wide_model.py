"""CPU: the recoding with a wide anchored window is exact (tests/anchor_wide_cases.py is the host model of csrc/partition.hpp next_digit).

For every scalar k < 2^bits(r):  sum over the entries of (sign) (bucket weight) 2^(position) + (the constant the host adds) == k, with no case
left out; a scalar with a bit at or above bits(r) is refused (the engine repeats it with the option off, where the same identity holds for
any 256-bit k).  BLS12-377's Fr has the wide window wherever c divides 252 (from c = 6 on) and BLS12-381's at no window size."""
import random

import pytest

import anchor_wide_cases as m


def test_where_the_wide_window_exists():
    assert [c for c in range(5, 24) if m.wide_fits(c, 253)] == [6, 7, 9, 12, 14, 18, 21]      # 252 = 2^2 3^2 7
    assert [c for c in range(5, 24) if m.wide_fits(c, 255)] == []


@pytest.mark.parametrize("c", [6, 7, 9, 12, 14, 18, 21])
def test_recoding_is_exact(c):
    rng = random.Random(c)
    ks = m.edge_scalars(c) + [rng.randrange(m.R377) for _ in range(8000)] + [rng.randrange(1 << 253) for _ in range(2000)]
    a = m.anchor_of(c, 253)
    seen_sets = set()
    for k in ks:
        ent, const = m.recode(k, c, 253, True)
        assert const == 1 << (c * a + c)
        assert m.value(ent, const, c, 253, True) == k, hex(k)
        assert len({g if g <= a else a for g, _, _ in ent}) == len(ent)      # one entry per DIGIT window at most
        assert len(ent) <= a + 1
        seen_sets.update(g for g, _, _ in ent)
        # the option off: round 6's anchored window, the same value
        ent0, const0 = m.recode(k, c, 253, False)
        assert const0 == 1 << (c * a + c - 1) and m.value(ent0, const0, c, 253, False) == k
    assert seen_sets == set(range(a + 2))          # both bucket sets of the wide window are in use


@pytest.mark.parametrize("c", [6, 12, 14, 18, 21])
def test_the_wide_windows_edges(c):
    a, full, half = m.anchor_of(c, 253), 1 << c, 1 << (c - 1)

    def top_entry(v):
        ent, _ = m.recode(v << (c * a), c, 253, True)
        return [e for e in ent if e[0] >= a]

    assert top_entry(full) == []                                   # s = 0: no entry
    assert top_entry(0) == [(a + 1, half, True)]                   # s = -2^c: the last bucket of the upper set
    assert top_entry(2 * full - 1) == [(a + 1, half - 1, False)]
    assert top_entry(full + half) == [(a, half, False)]            # magnitude 2^(c-1): still the lower set
    assert top_entry(full + half + 1) == [(a + 1, 1, False)]
    assert top_entry(full - half - 1) == [(a + 1, 1, True)]
    # v = 2^(c+1) itself: all ones and a carry
    ent, const = m.recode((1 << 253) - 1, c, 253, True)
    assert [e for e in ent if e[0] >= a] == [(a + 1, half, False)] and m.value(ent, const, c) == (1 << 253) - 1


def test_scalars_above_the_modulus_bits_are_refused_and_exact_without_the_option():
    rng = random.Random(7)
    for c in (12, 14, 18, 21):
        for k in [1 << 253, (1 << 256) - 1, (1 << 255) | 5, m.R377 << 3] + [rng.randrange(1 << 253, 1 << 256) for _ in range(500)]:
            assert m.recode(k, c, 253, True) is None
            ent, const = m.recode(k, c, 253, False)
            assert m.value(ent, const, c, 253, False) == k


def test_bls12_381_is_untouched():
    rng = random.Random(1)
    for k in [0, 1, m.R381 - 1, (1 << 255) - 1, (1 << 256) - 1] + [rng.randrange(1 << 256) for _ in range(500)]:
        assert m.recode(k, 17, 255, True) == m.recode(k, 17, 255, False)
        ent, const = m.recode(k, 17, 255, True)
        assert m.value(ent, const, 17, 255, True) == k
