"""The lean sweep's variant lists against its dispatch (no GPU): every listed
variant is reachable through a kernel spec (or, the y-marching thin-slab
forms, through a box shape), and every spec the dispatch accepts is listed."""
import itertools
import shutil


import _lean_variants as lv

DTYPES = ("fp64", "fp32")


def _supported_set(ext, dtype, with_source):
    """Every spec of the candidate grid that dispatch accepts, as list records."""
    out = set()
    for R, WY, K, Q, O, EW in itertools.product(range(2, 7), (8, 12, 16), range(2, 7), (3, 4, 6),
                                                (0, 2, 3, 17, 18, 19, 66), (0, 1, 3)):
        v = lv.Variant(dtype, R, WY, K, Q, O, False, EW, with_source)
        if ext.lean_supported(dtype, lv.spec(v), with_source):
            out.add(v)
    return out


def _listed_set(records, dtype, with_source):
    return {v for v in records if v.dtype == dtype and v.src == with_source and not v.SW}


def _mismatch(ext, records):
    """Specs listed but not dispatched, and dispatched but not listed."""
    dead, unlisted = [], []
    for dtype, with_source in itertools.product(DTYPES, (False, True)):
        have, want = _supported_set(ext, dtype, with_source), _listed_set(records, dtype, with_source)
        dead += sorted(lv.vid(v) + (" (source)" if with_source else "") for v in want - have)
        unlisted += sorted(lv.vid(v) + (" (source)" if with_source else "") for v in have - want)
    return dead, unlisted


def test_parser_finds_every_entry():
    """Counted two ways: the regex, and the lines that start with H3D_V."""
    texts = lv.list_text()
    lines = [lv.entry_lines(t) for t in texts]
    assert min(lines) > 0, lines
    assert [len(lv.parse(t)) for t in texts] == lines
    records = lv.variants()
    assert len(set(records)) == len(records), "duplicate entries"
    # the first list holds the plain and edge forms, the second the source forms
    assert not any(v.src for v in lv.parse(texts[0])) and all(v.src for v in lv.parse(texts[1]))


def test_every_listed_variant_is_dispatched(ext):
    for v in lv.variants():
        if v.SW:
            continue
        s = lv.spec(v)
        assert ext.lean_supported(v.dtype, s, v.src), f"{lv.vid(v)} is listed but dispatch does not reach it"
        # the spec names the variant itself: resolved() substitutes nothing
        r = [int(f) for f in ext.kernel_spec_resolved(s, v.dtype).split(":")[1:]] + [0, 0, 0]
        assert r[:6] == [1, v.R, 1, v.WY, 0, v.Q] and r[6] == v.NTS and r[8] == v.EW, (s, r)
        if v.EW:
            # the edge role: fp64 only, no source form
            assert v.dtype == "fp64" and not v.src
            assert not ext.lean_supported("fp32", s, False), s
            assert not ext.lean_supported("fp64", s, True) and not ext.lean_supported("fp32", s, True), s


def test_dispatch_and_lists_agree(ext):
    """Both directions over R 2..6, WY 8 / 12 / 16, K 2..6, Q 3 / 4 / 6, every
    store-policy value and edge role in use, V = 1: a listed variant that
    dispatch no longer reaches is dead compile time, a dispatched one that is
    not listed is a kernel no list-driven test launches."""
    dead, unlisted = _mismatch(ext, lv.variants())
    assert not dead, f"listed, not dispatched: {dead}"
    assert not unlisted, f"dispatched, not listed: {unlisted}"


def test_a_dropped_entry_is_noticed(ext, tmp_path):
    """The comparison itself: with one entry deleted from a copy of the lists,
    the spec it named is reported as dispatched but not listed."""
    for name in lv.LISTS:
        shutil.copy(f"{lv.KERNELS}/{name}", tmp_path / name)
    path = tmp_path / lv.LISTS[0]
    gone = "H3D_V(double, 3, 8, 6, 3, 0, false, 2)\n"
    text = path.read_text()
    assert text.count(gone) == 1
    path.write_text(text.replace(gone, ""))
    dead, unlisted = _mismatch(ext, lv.variants(str(tmp_path)))
    assert not dead and unlisted == ["fp64-tl6:1:3:1:8:0:3:0"], (dead, unlisted)


def test_thin_slab_forms_listed():
    """The y-marching forms are picked by box shape: the three tile shapes of
    lean_thin_slab, in both dtypes, with and without a source."""
    sw = [v for v in lv.variants() if v.SW]
    shapes = {(2, 5, 3), (3, 3, 3), (3, 4, 4)}
    assert {(v.dtype, v.src, (v.R, v.WY, v.K)) for v in sw} == set(itertools.product(DTYPES, (False, True), shapes))
    assert len(sw) == 12 and all(v.Q == 3 and v.EW == 0 and v.NTS == (2 if v.dtype == "fp64" else 0) for v in sw)


def _params(fn):
    """The parametrize marks of a test function as {argnames: values}."""
    return {m.args[0]: m.args[1] for m in fn.pytestmark if m.name == "parametrize"}


# the form each case of test_gpu_temporal.py's thin-slab tests is there for
# (R, WY, K of the y-marching tile; None: the x-marching tile its docstring names)
THIN_K3 = {(12, (0, 3), "both", 64): (3, 3, 3), (12, (9, 12), "both", 64): (3, 3, 3), (6, (0, 3), "lo", 100): (3, 3, 3),
           (9, (6, 9), "hi", 49): (3, 3, 3), (20, (0, 4), "both", 70): (2, 5, 3), (8, (0, 6), "both", 130): (3, 3, 3)}
THIN_K4 = {(12, (0, 4), "both", 64): (3, 4, 4), (12, (8, 12), "both", 64): (3, 4, 4), (9, (0, 4), "lo", 100): (3, 4, 4),
           (9, (5, 9), "hi", 70): (3, 4, 4), (20, (0, 3), "both", 70): (3, 4, 4),
           (20, (16, 20), "both", 63): None}  # ny < 16 x planes: the x-marching default, as its docstring says


def test_thin_slab_cases_meet_their_dispatch_predicate():
    """test_sweep_thin_slab_y_marching[_k4] compare with the CPU sweep whatever
    kernel ran; by the boxes' shapes, each case reaches the y-marching form it
    is there for (a case that fell through to the x-marching tile would test
    nothing new), and together they reach every listed thin-slab shape."""
    import test_gpu_temporal as t

    reached = set()
    for fn, K, table in ((t.test_sweep_thin_slab_y_marching, 3, THIN_K3),
                         (t.test_sweep_thin_slab_y_marching_k4, 4, THIN_K4)):
        p = _params(fn)
        cases = [tuple(c) for c in p["n0,box_x,side,ny"]]
        assert set(cases) == set(table), "a thin-slab case was added or changed: state the form it is there for"
        kernels = p.get("kernel", ["tl4"])
        assert f"tl{K}" in kernels  # the default spec, which alone takes the y-marching forms
        for n0, box_x, side, ny in cases:
            # _deep_halo_case: the box spans every row, box_x in x
            assert 0 <= box_x[0] < box_x[1] <= n0
            form = lv.thin_slab_form(K, box_x[1] - box_x[0], ny)
            assert form == table[(n0, box_x, side, ny)], (K, n0, box_x, side, ny, form)
            reached.add(form)
        assert all(lv.thin_slab_form(K, 4, 64, default_spec=(k == f"tl{K}")) is None for k in kernels if k != f"tl{K}")
        assert set(p["dtype"]) == {t.torch.float64, t.torch.float32}
    assert reached - {None} == {(v.R, v.WY, v.K) for v in lv.variants() if v.SW}
