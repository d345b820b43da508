"""The GEMM planner (mp_gemm_plan, gemm_bf16.hip gemm_plan): a pure host function - these tests run without a GPU, through ctypes, with the
MI355X's 256 CUs given explicitly.

What they hold: (a) every Linear shape of the headline run plans what ran before the planner existed (persistent 256 x 256 kernel, 256
workgroups); (b) at the reference's own batch sizes the plan is what the committed crossover measurement says; (c) no plan violates a
kernel's preconditions, over a sweep of shapes; (d) the gemm_tile option."""
import ctypes as C

import pytest

from manipose_amd import _lib

TOK = 243 * 17                                # tokens of one window
LAYERS = {"qkv": (1536, 512), "proj": (512, 512), "fc1": (2048, 512), "fc2": (512, 2048)}      # Linear(K -> N) as (N, K)
CUS = 256
EPI_BIAS, EPI_GELU, EPI_RESID, EPI_DGELU, EPI_SLAB = range(5)
FWD_EPI = {"qkv": EPI_BIAS, "proj": EPI_RESID, "fc1": EPI_GELU, "fc2": EPI_RESID}


@pytest.fixture(scope="module")
def lib():
    lib = _lib.load()
    assert lib.mp_set_option(b"gemm_tile", 0) == 0
    return lib


def plan(lib, M, N, K, form, epi, cus=CUS):
    out = (C.c_int * 4)()
    rc = lib.mp_gemm_plan(M, N, K, form, epi, cus, out)
    return rc, tuple(out)


def gemm_of(form, layer):
    """(N, K, epilogue) of the GEMM the crossover log measured for this operand form and layer: the forward Linear for f16f8 (8) and bf16x3 (1),
    the dgrad dx = dy W for plain bf16 (0) - a GEMM with N = the layer's inputs, K = its outputs, the fc2 one multiplying gelu'."""
    N, K = LAYERS[layer]
    if form == 0:
        return K, N, (EPI_DGELU if layer == "fc2" else EPI_BIAS)
    return N, K, FWD_EPI[layer]


@pytest.mark.parametrize("form", [8, 1, 0])
@pytest.mark.parametrize("B", [79, 118, 158, 198])
def test_headline_shapes_plan_what_ran_before(lib, B, form):
    """B = 158 is the headline batch; 79 / 118 / 198 the other timed ones: the persistent kernel on 256 workgroups, for every layer and form."""
    for layer, (N, K) in LAYERS.items():
        rc, p = plan(lib, B * TOK, N, K, form, FWD_EPI[layer])
        assert rc == 0 and p[:3] == (256, 1, 256), (layer, p)
        assert p[3] == -(-B * TOK // 256) * (N // 256)
        N2, K2, epi = gemm_of(form, layer)
        rc, p = plan(lib, B * TOK, N2, K2, form, epi)
        assert rc == 0 and p[:3] == (256, 1, 256), (layer, p)


# (form, windows, layer) -> (plan_tile, plan_persistent, measured t128 / t256): copied from profiles/small_batch/crossover.log (the rows of
# M = 4131 x 1, 3, 10, 25; form 8 = its f16f8 table, 1 = its x3 table, 0 = its bf16 dgrad table).  For the shapes the older forms' persistent
# kernel serves (plan_persistent 1) the ratio compares the tiled 128 kernel with the persistent one.
TABLE = {
    (8, 1, "qkv"): (128, 0, 0.775), (8, 1, "proj"): (128, 0, 0.586), (8, 1, "fc1"): (256, 1, 1.275), (8, 1, "fc2"): (128, 0, 0.741),
    (8, 3, "qkv"): (256, 1, 1.161), (8, 3, "proj"): (128, 0, 0.640), (8, 3, "fc1"): (256, 1, 1.291), (8, 3, "fc2"): (128, 0, 0.720),
    (8, 10, "qkv"): (256, 1, 1.576), (8, 10, "proj"): (256, 1, 0.958), (8, 10, "fc1"): (256, 1, 1.387), (8, 10, "fc2"): (256, 1, 1.134),
    (8, 25, "qkv"): (256, 1, 1.486), (8, 25, "proj"): (256, 1, 1.131), (8, 25, "fc1"): (256, 1, 1.396), (8, 25, "fc2"): (256, 1, 1.274),
    (1, 1, "qkv"): (128, 0, 0.653), (1, 1, "proj"): (128, 0, 0.491), (1, 1, "fc1"): (256, 0, 0.941), (1, 1, "fc2"): (128, 0, 0.478),
    (1, 3, "qkv"): (128, 0, 0.732), (1, 3, "proj"): (128, 0, 0.604), (1, 3, "fc1"): (256, 0, 0.962), (1, 3, "fc2"): (128, 0, 0.598),
    (1, 10, "qkv"): (256, 1, 1.354), (1, 10, "proj"): (128, 0, 0.807), (1, 10, "fc1"): (256, 1, 1.265), (1, 10, "fc2"): (128, 0, 0.911),
    (1, 25, "qkv"): (256, 1, 1.304), (1, 25, "proj"): (256, 1, 1.258), (1, 25, "fc1"): (256, 1, 1.328), (1, 25, "fc2"): (256, 1, 1.239),
    (0, 1, "qkv"): (128, 0, 0.504), (0, 1, "proj"): (128, 0, 0.539), (0, 1, "fc1"): (128, 0, 0.497), (0, 1, "fc2"): (256, 0, 1.018),
    (0, 3, "qkv"): (128, 0, 0.611), (0, 3, "proj"): (128, 0, 0.651), (0, 3, "fc1"): (128, 0, 0.621), (0, 3, "fc2"): (256, 0, 1.003),
    (0, 10, "qkv"): (128, 0, 0.864), (0, 10, "proj"): (128, 0, 0.850), (0, 10, "fc1"): (128, 0, 0.878), (0, 10, "fc2"): (256, 1, 1.690),
    (0, 25, "qkv"): (256, 1, 1.228), (0, 25, "proj"): (256, 1, 1.204), (0, 25, "fc1"): (256, 1, 1.255), (0, 25, "fc2"): (256, 1, 1.810),
}


@pytest.mark.parametrize("form", [8, 1, 0])
@pytest.mark.parametrize("B", [1, 3, 10, 25])
def test_small_batches_plan_what_the_crossover_table_says(lib, B, form):
    for layer in LAYERS:
        tile, persistent, ratio = TABLE[(form, B, layer)]
        N, K, epi = gemm_of(form, layer)
        rc, p = plan(lib, B * TOK, N, K, form, epi)
        assert rc == 0 and p[:2] == (tile, persistent), (form, B, layer, p)
        # ... and the table agrees with its own timings: the small tile where it was measured faster, the large one where the small one
        # was slower or within the planner's 10 % margin
        if tile == 128:
            assert ratio < 1.0, (form, B, layer, ratio)
        elif not persistent or form == 8:
            assert ratio > 1 / 1.10, (form, B, layer, ratio)


def test_the_table_holds_a_small_tile_choice_among_the_f16f8_layers_at_B3():
    """the feature: with none, the 128 x 128 f16f8 kernel would never run at the reference's default batch"""
    small = [layer for layer in LAYERS if TABLE[(8, 3, layer)][0] == 128]
    assert small, "no f16f8 layer plans the small tile at B = 3"
    assert set(small) == {"proj", "fc2"}      # 98 large tiles for 256 CUs (the fill arithmetic); qkv and fc1 need 3 / 4 rounds of small tiles against 2


def _ms():
    ms = set(range(1, 600))
    for base in range(0, 70000, 256 * 7):
        for off in (0, 1, 127, 128, 129, 255):
            ms.add(base + off)
    ms |= {4131, 12393, 41310, 65535, 65536, 69999, 70000}
    return sorted(m for m in ms if 1 <= m <= 70000)


@pytest.mark.parametrize("form", [8, 1, 0, 16])
def test_no_plan_violates_a_precondition(lib, form):
    ms = _ms()
    assert {m % 128 for m in ms} >= {0, 1, 127} and {m % 256 for m in ms} >= {0, 1, 127, 255}
    for N in (128, 256, 384, 512, 1536, 2048):
        for K in (64, 128, 512, 2048):
            for epi in (EPI_BIAS, EPI_GELU, EPI_RESID):
                for M in ms:
                    rc, (tile, persistent, wgs, tiles) = plan(lib, M, N, K, form, epi)
                    if form == 8 and (N % 256 != 0 or K % 64 != 0 or K < 128):
                        assert rc != 0, (M, N, K, "f16f8 planned outside its preconditions")
                        continue
                    assert rc == 0, (M, N, K, form, epi)
                    assert tile in (128, 256) and persistent in (0, 1) and wgs >= 1
                    assert tiles == -(-M // tile) * -(-N // tile), (M, N, K, tile, tiles)
                    if persistent:
                        assert tile == 256 and K >= 128 and K % 64 == 0 and N % 256 == 0, (M, N, K)
                        assert wgs <= CUS and wgs % 8 == 0
                    else:
                        assert wgs == tiles
                    if tile == 256:
                        assert N % 256 == 0 and (M >= 256 or form == 8), (M, N, K)
                    if form == 8 and tile == 128:
                        assert not persistent


def test_the_small_tile_is_never_planned_from_two_large_tiles_per_cu_up(lib):
    for form in (8, 1, 0, 16):
        for N, K in LAYERS.values():
            for M in range(256 * 2 * CUS * 256 // N, 700000, 50021):
                rc, p = plan(lib, M, N, K, form, EPI_BIAS)
                assert rc == 0 and p[0] == 256, (form, M, N, p)


def test_gemm_tile_option(lib):
    try:
        assert lib.mp_set_option(b"gemm_tile", 64) != 0
        assert b"gemm_tile" in lib.mp_last_error()
        assert lib.mp_set_option(b"gemm_tile", 256) == 0
        for form in (8, 1, 0, 16):
            for N in (128, 256, 384, 512, 1536, 2048):
                for M in (17, 255, 256, 4131, 12393, 41310):
                    rc, p = plan(lib, M, N, 512, form, EPI_BIAS)
                    has256 = N % 256 == 0 and (M >= 256 or form == 8)      # (the f16f8 persistent kernel takes any M; the tiled template wants one full tile)
                    if form == 8 and N % 256:
                        assert rc != 0
                    else:
                        assert rc == 0 and p[0] == (256 if has256 else 128), (form, M, N, p)
        assert lib.mp_set_option(b"gemm_tile", 128) == 0
        for form in (8, 1, 0, 16):
            for M in (4131, 12393, 652698):
                rc, p = plan(lib, M, 512, 512, form, EPI_BIAS)
                assert rc == 0 and p[:2] == (128, 0), (form, M, p)
        # the weight-gradient launches keep the tile their split-K was laid out for
        rc, p = plan(lib, 512, 512, 12393, 0, EPI_SLAB)
        assert rc == 0 and p[:2] == (256, 0), p
    finally:
        assert lib.mp_set_option(b"gemm_tile", 0) == 0


def test_older_hooks_keep_their_meaning(lib):
    """gemm_small_tile forces 128 for the forms that had a small tile before the planner and does nothing to f16f8; gemm_persist_min_tiles > 0 sends
    every qualifying shape - three windows included - to the persistent kernel."""
    M = 3 * TOK
    try:
        assert lib.mp_set_option(b"gemm_small_tile", 1) == 0
        assert plan(lib, M, 512, 512, 1, EPI_RESID)[1][:2] == (128, 0)
        assert plan(lib, 158 * TOK, 512, 512, 0, EPI_BIAS)[1][:2] == (128, 0)
        assert plan(lib, 158 * TOK, 512, 512, 8, EPI_RESID)[1][:3] == (256, 1, 256)
        assert plan(lib, M, 1536, 512, 8, EPI_BIAS)[1][:2] == (256, 1)
        assert lib.mp_set_option(b"gemm_small_tile", 0) == 0
        assert lib.mp_set_option(b"gemm_persist_min_tiles", 1) == 0
        for form in (8, 1, 0):
            for layer, (N, K) in LAYERS.items():
                assert plan(lib, M, N, K, form, FWD_EPI[layer])[1][:3] == (256, 1, 256), (form, layer)
    finally:
        assert lib.mp_set_option(b"gemm_small_tile", 0) == 0
        assert lib.mp_set_option(b"gemm_persist_min_tiles", 0) == 0


def test_launch_counters_exist_and_reset(lib):
    out = (C.c_int64 * 3)()
    assert lib.mp_gemm_launch_counts(out, 1) == 0
    assert lib.mp_gemm_launch_counts(out, 0) == 0 and list(out) == [0, 0, 0]
