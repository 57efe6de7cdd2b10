"""The baby-step / giant-step plan of device.lin_transform without a device: the diagonals of a
matrix, the rotation keys a plan needs, and the plans that are refused.  The plan is checked for its meaning in
numpy: rolled diagonals against baby rotations, turned by the giant step, sum to M @ x."""
import numpy as np
import pytest

from SHELFI_FHE import device as D


def _apply(diags, babies, x):
    """lin_transform's arithmetic on a plain vector, np.roll(x, -r) standing for the rotation by r."""
    batch, b, plan = D._lin_plan(diags, babies)
    y = np.zeros(batch)
    for G, steps in plan.items():
        assert G % b == 0 and all(0 <= i < b for i in steps)
        part = sum(np.roll(diags[d], G) * np.roll(x, -i) for i, d in steps.items())
        y += np.roll(part, -G)
    return y


@pytest.mark.parametrize("babies", [None, 1, 2, 4, 16])
def test_plan_computes_the_matrix_product(babies):
    rng = np.random.default_rng(7)
    M = rng.uniform(-1, 1, (16, 16))
    x = rng.uniform(-1, 1, 16)
    diags = D.diagonals(M)
    assert sorted(diags) == list(range(16))
    assert np.allclose(_apply(diags, babies, x), M @ x, atol=1e-12)
    band = np.zeros((16, 16))
    s = np.arange(16)
    for d in (-1, 0, 1):
        band[s, (s + d) % 16] = rng.uniform(-1, 1, 16)
    bd = D.diagonals(band)
    assert sorted(bd) == [0, 1, 15]
    assert np.allclose(_apply(bd, babies, x), band @ x, atol=1e-12)


def test_indices_are_the_plans_rotations():
    v = np.ones(16)
    assert D.lin_transform_indices({d: v for d in range(16)}, 4) == [1, 2, 3, 4, 8, 12]
    assert D.lin_transform_indices({d: v for d in range(16)}) == [1, 2, 3, 4, 8, 12]  # sqrt(16)
    assert D.lin_transform_indices({0: v, 1: v, 15: v}) == [-2, 1]  # a band is centred: span 3, b = 2
    assert D.lin_transform_indices({0: v, 1: v, -1: v}) == [-2, 1]
    assert D.lin_transform_indices({0: v}) == []
    assert D.lin_transform_indices({5: v}, 4) == [1, 4]


def test_refused_plans():
    v = np.ones(4096)
    with pytest.raises(ValueError, match="b = 1 with 70 giant"):
        D.lin_transform_indices({d: v for d in range(70)}, babies=1)
    assert len(D.lin_transform_indices({d: v for d in range(70)})) == 7 + 8  # b = 8: babies 1..7, giants 8..64
    with pytest.raises(ValueError):
        D.lin_transform_indices({0: v, 4096: v})  # the same diagonal twice
    with pytest.raises(ValueError):
        D.lin_transform_indices({0: v}, babies=3)
    with pytest.raises(ValueError):
        D.lin_transform_indices({0: v, 1: v[:5]})
    with pytest.raises(ValueError):
        D.lin_transform_indices({})
    with pytest.raises(ValueError):
        D.diagonals(np.ones((3, 4)))
