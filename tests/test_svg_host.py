"""gsdf_amd/svg.py: write followed by read is bit-exact -- subnormals, negative zero, values that need all nine digits -- the
shortest decimal is what is written, one even-odd path per layer (empty layers included), the y axis turned by a transform."""
import re

import numpy as np
import pytest

from gsdf_amd import svg

F = np.float32


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def awkward_values():
    rng = np.random.default_rng(11)
    special = np.array([0.0, -0.0, 1e-45, -1e-45, 1.1754942e-38, 1.17549435e-38, 3.4028235e38, -3.4028235e38, 0.1, 1 / 3, 16777217.0, 8388608.5,
                        0.3, 123456.79, 1e-10, 9.99999994e-9, 1.00000012], np.float64).astype(F)
    random_bits = rng.integers(0, 2 ** 32, 4000, dtype=np.uint64).astype(np.uint32).view(F)
    random_bits = random_bits[np.isfinite(random_bits)]
    v = np.concatenate([special, random_bits, np.nextafter(F(1), F(2), dtype=F).reshape(1)]).astype(F)
    return v[: len(v) // 2 * 2]


def test_shortest_decimal_round_trips():
    for v in awkward_values():
        s = svg.fmt(v)
        assert (bits(np.array([float(s)]).astype(F)) == bits(v)).all(), (s, v)
        mant = re.sub(r"[eE].*$", "", s).replace("-", "").replace(".", "").lstrip("0")
        assert len(mant) <= 9, s
    assert svg.fmt(F(0.1)) == "0.1" and svg.fmt(F(-0.0)) == "-0" and svg.fmt(F(2.5)) == "2.5" and svg.fmt(F(1e-45)) == "1e-45"
    for bad in (float("nan"), float("inf"), float("-inf")):
        with pytest.raises(ValueError):
            svg.fmt(bad)


def test_write_then_read_is_bit_exact(tmp_path):
    v = awkward_values().reshape(-1, 2)
    layers = [[v[:5], v[5:400]], [], [v[400:]], [np.array([[0, 0], [1, 0], [1, 1], [0, 1]], F), np.array([[0.25, 0.25], [0.25, 0.75], [0.75, 0.75], [0.75, 0.25]], F)]]
    z = np.array([0.05, 0.15, 0.25, 0.35], F)
    p = tmp_path / "a.svg"
    svg.write_svg(str(p), layers, z=z)
    back = svg.read_svg(str(p))
    assert [len(l) for l in back] == [2, 0, 1, 2]
    for a, b in zip(layers, back):
        for la, lb in zip(a, b):
            assert lb.dtype == np.float32 and lb.shape == la.shape and (bits(la) == bits(lb)).all()
    text = p.read_text()
    paths = re.findall(r"<path\b[^>]*>", text)
    assert len(paths) == 4 and all('fill-rule="evenodd"' in t for t in paths)
    assert [t.count("M ") for t in paths] == [2, 0, 1, 2] and [t.count(" Z") for t in paths] == [2, 0, 1, 2]
    assert 'data-z="0.05"' in paths[0] and 'data-z="0.35"' in paths[3]
    # the y axis is turned by the group's transform; the coordinates are the part's own
    assert 'transform="scale(1,-1)"' in text and "M 0 0 L 1 0 L 1 1 L 0 1 Z" in text
    vb = [float(x) for x in re.search(r'viewBox="([^"]*)"', text).group(1).split()]
    assert vb[1] < 0 < vb[3]


def test_no_loops_at_all(tmp_path):
    p = tmp_path / "e.svg"
    svg.write_svg(str(p), [[]])
    assert svg.read_svg(str(p)) == [[]]
