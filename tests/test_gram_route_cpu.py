"""The route of a Gram launch (blsq_debug_gram_route: decided on the host, no GPU needed) under the default switches.

The library's central promise is that a problem's summation order — and so every bit of its result — depends on its
shape (m, n) and never on the batch it shares a launch with.  The GPU tests prove three order classes bit-identical
on sample shapes: the direct kernel per template instance, the k-split kernel of eight column tiles per instance, and
the tile table shared by gram1, gram16 and the generic kernel.  Here the class, rows_per_chunk and rhs_valu are checked
to be functions of (m, n) alone over every n <= 271."""
import ctypes as C

import pytest

DIRECT, GRAM8, GRAM1, GRAM16, GENERIC = range(5)
LDS_MAX = 160 * 1024                       # one workgroup's LDS on CDNA4

M_VALUES = (None, 512, 2048, 2049, 4096, 131072, 131073, 250000)      # None: m = n
B_VALUES = (1, 2, 4, 5, 64, 65, 255, 256, 512, 1024)

# The kernel instances the library builds: the dispatch table of launch_gram (gram_kernels.hip).
INSTANCES = {
    DIRECT: {(ntt, rhs, nwd) for ntt in (1, 2, 3, 4) for rhs in (0, 1) for nwd in (2, 4, 8)},
    GRAM8: {(0, 0, 0), (1, 0, 0)},
    GRAM1: {(0, 0, 0)},
    GRAM16: {(rhs, pair, 0) for rhs in (0, 1) for pair in (0, 1)},
    GENERIC: {(sl, cb, 0) for sl, cbs in ((1, (1, 2, 5)), (2, (1, 2, 5)), (4, (1, 2, 5)), (8, (2, 3, 5)),
                                          (12, (3, 4, 5)), (17, (4, 5)), (20, (4, 5))) for cb in cbs},
}


def _route(lib, m, n, B, has_final=1):
    out = (C.c_int32 * 16)()
    assert lib.blsq_debug_gram_route(None, m, n, B, has_final, out) == 0, (m, n, B)
    v = list(out)
    return {"family": v[0], "key": tuple(v[1:4]), "grid": tuple(v[4:7]), "block": v[7], "lds": v[8],
            "rhs_valu": v[9], "rows_per_chunk": v[10], "tile_groups": v[11], "fused": v[12], "chunks": v[13]}


def _order_class(r):
    if r["family"] == DIRECT:
        return ("direct",) + r["key"]
    if r["family"] == GRAM8:
        return ("gram8", r["key"][0])
    return ("tile table",)


@pytest.fixture(scope="module")
def lib():
    from bounded_lsq import _abi
    return _abi.load()


def _shapes():
    for n in range(1, 272):
        for m in sorted({n if mv is None else mv for mv in M_VALUES}):
            if m >= n:
                yield m, n


def test_order_class_does_not_depend_on_the_batch(lib):
    nroutes = 0
    for m, n in _shapes():
        for has_final in (0, 1):
            seen = {}
            for B in B_VALUES:
                r = _route(lib, m, n, B, has_final)
                nroutes += 1
                seen[B] = (_order_class(r), r["rows_per_chunk"], r["rhs_valu"])
            assert len(set(seen.values())) == 1, (m, n, has_final, seen)
    assert nroutes == 2 * len(B_VALUES) * len(list(_shapes())) > 40000


def test_every_route_fits_a_workgroup_and_names_a_built_instance(lib):
    for m, n in _shapes():
        for B in B_VALUES:
            for has_final in (0, 1):
                r = _route(lib, m, n, B, has_final)
                assert 0 <= r["lds"] <= LDS_MAX, (m, n, B, r)
                assert r["family"] in INSTANCES and r["key"] in INSTANCES[r["family"]], (m, n, B, r)
                assert 1 <= r["block"] <= 1024 and min(r["grid"]) >= 1, (m, n, B, r)
                assert r["fused"] == (1 if r["family"] == GRAM16 and r["key"][1] else 0), (m, n, B, r)


def test_pinned_routes(lib):
    # 4096 x 256, a full batch: sixteen column tiles, static tile rows per wave, rhs beside the tiles; with the final
    # slot on offer both row chunks go to one workgroup, which sums them itself
    r = _route(lib, 4096, 256, 512, has_final=1)
    assert (r["family"], r["key"], r["grid"], r["fused"]) == (GRAM16, (1, 1, 0), (1, 512, 1), 1)
    assert (r["rhs_valu"], r["rows_per_chunk"], r["chunks"], r["block"]) == (1, 2048, 2, 512)
    r = _route(lib, 4096, 256, 512, has_final=0)
    assert (r["family"], r["key"], r["grid"], r["fused"]) == (GRAM16, (1, 0, 0), (2, 512, 1), 0)
    # ... and ONE such problem: a tile per wave straight from global memory
    assert _route(lib, 4096, 256, 1)["family"] == GRAM1
    # 512 x 64: the direct kernel, four column tiles of J^T J, rhs from the same fragments, two waves (<= 512 rows)
    r = _route(lib, 512, 64, 1024)
    assert (r["family"], r["key"], r["grid"], r["block"]) == (DIRECT, (4, 1, 2), (1, 1024, 1), 128)
    # n = 120: eight column tiles, the k-split kernel whatever the batch
    for B in (1, 1024):
        r = _route(lib, 4096, 120, B)
        assert (r["family"], r["key"]) == (GRAM8, (0, 0, 0)), r
    # n = 257: seventeen column tiles, 153 tiles on eight waves: twenty slots, five column blocks of 64
    r = _route(lib, 4096, 257, 512)
    assert (r["family"], r["key"], r["tile_groups"]) == (GENERIC, (20, 5, 0), 1)


def test_unsupported_shapes_are_refused(lib):
    out = (C.c_int32 * 16)()
    assert lib.blsq_debug_gram_route(None, 4096, 272, 1, 0, out) != 0      # eighteen column tiles
    assert lib.blsq_debug_gram_route(None, 8, 16, 1, 0, out) != 0          # m < n
    assert lib.blsq_debug_gram_route(None, 4096, 64, 0, 0, out) != 0
