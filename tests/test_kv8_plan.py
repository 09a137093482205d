"""CPU tests of the plan universe of the fp8-KV-cache units (tests/kv8_plan_universe.py): the table against the kernel symbols
of the compiled device code of csrc/fa_fwd_kv8_api.hip, csrc/fa_fwd_qv8_api.hip and csrc/fa_kvcache_append_kv8.hip, the plan of
every GPU case (fa_fwd_kv8_plan_name / fa_fwd_qv8_plan_name), and the geometry the cases and the edge set of
tests/test_kv8_plan_parity_gpu.py promise, through the module's replay of the kernels' key-range arithmetic.  Nothing here
touches a device."""
import importlib
import re

import pytest

import kv8_plan_universe as U
import layouts
from device_asm import TYPES, fp8_cache_kernels, kernel_bodies
from flash_attention_annotated_amd import _lib
from parity_helpers import plan_key
from test_kv8_abi import ADDR, _params as kv8_params
from test_qv8_abi import _params as qv8_params

UNITS = {"kv8": ("fa_fwd_kv8_api.hip", "kv8_fwd_kernel", "PkParams", "D"), "qv8": ("fa_fwd_qv8_api.hip", "qv8_fwd_kernel", "QvParams", "DVT")}
DTYPE = {"bf16": _lib.FA_DTYPE_BF16, "fp16": _lib.FA_DTYPE_FP16}
CASES = U.cases()
IDS = [U.case_id(f, ep, dt) for f, ep, dt, _ in CASES]


# ---- the universe against the compiler -------------------------------------------------------------------------------------
def test_universe_is_every_compiled_kernel_of_the_two_forward_units():
    """The (type, form) pairs of UNIVERSE are exactly the kernels of the device code of fa_fwd_kv8_api.hip and
    fa_fwd_qv8_api.hip, each with both epilogues: an instantiation added to either unit without a row fails here, and so does
    a row whose kernel is gone (a kernel of another name in either unit fails in the parser)."""
    compiled = set()
    for unit, kernel, params, n in UNITS.values():
        for dt, width, softcap in fp8_cache_kernels(unit, kernel, params):
            compiled.add((dt, f"{kernel} {n}={width} waves=4" + (" SOFTCAP" if softcap else "")))
    assert len(compiled) == 16
    listed = {(dt, form) for dt, form, _ in U.UNIVERSE}
    assert compiled == listed, (sorted(compiled - listed), sorted(listed - compiled))
    assert set(U.UNIVERSE) == {(dt, form, ep) for dt, form in compiled for ep in U.EPILOGUES} and len(U.UNIVERSE) == 32
    ids = [U.case_id(form, ep, dt) for form, ep, dt, _ in U.cases()]
    assert len(set(ids)) == len(ids) == len(U.UNIVERSE) - len(U.UNREACHABLE) * len(U.DTYPES)
    assert not [k for k in U.UNREACHABLE if k[1] in U.FORMS.get(k[0], {})], "a case and an UNREACHABLE rule for one key"
    # no rule forbids a key today: test_universe_case_is_planned_on_its_key plans all 32.  A key listed here needs its rule
    # asserted here as well, as tests/test_fwd_plan.py does for plan_universe.UNREACHABLE
    assert U.UNREACHABLE == {}


def test_aux_is_every_kernel_of_the_append_unit():
    """kvcache_append_kv8_kernel is the only kernel of fa_kvcache_append_kv8.hip, in exactly the AUX element types, and the
    GPU test AUX names exists."""
    compiled = set()
    for sym, _ in kernel_bodies("fa_kvcache_append_kv8.hip"):
        m = re.match(r"_ZN\d+_GLOBAL__N_1(\d+)", sym)
        assert m, sym
        name, rest = sym[m.end():m.end() + int(m.group(1))], sym[m.end() + int(m.group(1)):]
        t = re.match(r"I(DF16b|DF16_)E", rest)
        assert t, sym
        compiled.add((name, TYPES[t.group(1)]))
    listed = {(name, dt) for name, (_, types) in U.AUX.items() for dt in types}
    assert compiled == listed == {("kvcache_append_kv8_kernel", "bf16"), ("kvcache_append_kv8_kernel", "fp16")}
    for where, _ in U.AUX.values():
        path, _, name = where.partition("::")
        assert path.startswith("tests/") and path.endswith("_gpu.py"), path
        module = importlib.import_module(path[len("tests/"):-len(".py")])
        assert callable(getattr(module, name, None)), f"{where} does not exist"
        marks = getattr(module, "pytestmark", None)
        assert "gpu" in [m.name for m in (marks if isinstance(marks, list) else [marks]) if m is not None]


# ---- planning -----------------------------------------------------------------------------------------------------------------
def _case_params(case, dt):
    """The universe case as the FA3 binding hands it to fa_fwd_kv8 / fa_fwd_qv8: the capacity as seqlen_k, the fill levels and
    both descales as device pointers, the FA3 window rule."""
    kw = dict(b=case["b"], h=case["h"], h_k=case["hk"], sq=case["sq"], sk=case["cap"], d=case["d"], dtype=DTYPE[dt],
              is_causal=int(case["causal"]), softcap=case.get("softcap", 0.0), num_splits=case["splits"], seqused_k=ADDR,
              k_descale=ADDR, v_descale=ADDR, k_descale_batch_stride=case["hk"], k_descale_head_stride=1,
              v_descale_batch_stride=case["hk"], v_descale_head_stride=1, flags=_lib.FA_FLAG_FA3_WINDOW)
    if case["kernel"] == "qv8":
        return qv8_params(dv=case["dv"], **kw)
    return kv8_params(**kw)


@pytest.mark.parametrize("form,ep,dt,case", CASES, ids=IDS)
def test_universe_case_is_planned_on_its_key(form, ep, dt, case):
    """Every GPU case is planned on exactly its key.  The plan text does not carry the element type: the type is what the params
    hold (the launch picks the instantiation by p->dtype alone), so both types count as keys through them."""
    lib = _lib.load()
    p = _case_params(case, dt)
    validate, plan_name = ((lib.fa_fwd_kv8_validate, lib.fa_fwd_kv8_plan_name) if case["kernel"] == "kv8" else
                           (lib.fa_fwd_qv8_validate, lib.fa_fwd_qv8_plan_name))
    assert validate(p) == 0
    name = plan_name(p, 256).decode()
    assert p.dtype == DTYPE[dt] and plan_key(name, dt) == (dt, form, ep), name
    assert form.startswith(case["kernel"] + "_fwd_kernel")
    assert int(re.search(r"block_m=(\d+)", name).group(1)) == U.block_m(case["kernel"])
    assert int(re.search(r"splits=(\d+)", name).group(1)) == case["splits"] == (3 if ep == "partial" else 1)


# layouts either plan legitimately moves to another form: (form, epilogue, assignment) -> (form, the rule's text).  None: plan_kv8 /
# plan_qv8 read no stride.
LAYOUT_MOVES = {}


@pytest.mark.parametrize("assignment", range(len(layouts.ASSIGNMENTS)))
@pytest.mark.parametrize("form,ep,dt,case", CASES, ids=IDS)
def test_universe_case_keeps_its_plan_on_strided_operands(form, ep, dt, case, assignment):
    """The plan text is the same when the strides of a case are those of a mixed assignment of tests/layouts.py: q / o / qv in
    elements, the cache in bytes, the descales transposed."""
    lib = _lib.load()
    p = _case_params(case, dt)
    validate, plan_name = ((lib.fa_fwd_kv8_validate, lib.fa_fwd_kv8_plan_name) if case["kernel"] == "kv8" else
                           (lib.fa_fwd_qv8_validate, lib.fa_fwd_qv8_plan_name))
    want = plan_name(p, 256).decode()
    a, b, dv = layouts.ASSIGNMENTS[assignment], case["b"], case.get("dv", case["d"])
    shapes = dict(q=(b, case["sq"], case["h"], case["d"]), k=(b, case["cap"], case["hk"], case["d"]), v=(b, case["cap"], case["hk"], dv),
                  o=(b, case["sq"], case["h"], dv), qv=(b, case["sq"], case["h"], dv))
    for n, shape in shapes.items():
        if n == "qv" and case["kernel"] != "qv8":
            continue
        for field, stride in zip(("batch", "row", "head"), layouts.geometry(shape, 1 if n in "kv" else 2, a[n])[2]):
            setattr(p, f"{n}_{field}_stride", stride)
    p.k_descale_batch_stride, p.k_descale_head_stride, p.v_descale_batch_stride, p.v_descale_head_stride = 1, b + 3, case["hk"] + 3, 1
    assert validate(p) == 0
    name = plan_name(p, 256).decode()
    assert LAYOUT_MOVES.get((form, ep, assignment)) is None and name == want, f"{name!r}, {want!r} on contiguous operands"


# ---- geometry -----------------------------------------------------------------------------------------------------------------
def _check_geometry(form, ep, case):
    """The conditions of the module docstring; raises AssertionError naming the one that breaks."""
    block, g, sq, lens = U.block_m(case["kernel"]), case["h"] // case["hk"], case["sq"], case["lens"]
    assert case["causal"] and case["cap"] >= max(lens) and case["b"] == len(lens)
    assert all(n % 64 != 0 for n in lens), "a ragged last tile in every entry"
    assert len(set(lens)) == len(lens), "fill levels differ between the batch entries"
    assert case["hk"] >= 2 and g & (g - 1) != 0, "h_k >= 2 and a GQA group that is no power of two"
    prows = sq * g
    assert prows > block and prows % block != 0, "a second row block with a short tail"
    assert block % g != 0 and 32 % g != 0, "block and wave edges cut a head group"
    width = case["d"] if case["kernel"] == "kv8" else case["dv"]
    assert f"={width} " in form, "every column of the tile carries data"
    sk = max(lens)
    blocks = U.replay(sq, sk, g, block, causal=True, splits=case["splits"])
    assert len(blocks) == -(-prows // block) >= 2
    rows = [r for blk in blocks for r in blk["rows"]]
    assert all(lo < hi for _, lo, hi in rows), "every row sees keys"
    untouched = min(hi for _, _, hi in rows) // 64
    assert untouched >= 3 and max(lo for _, lo, _ in rows) == 0, "three full tiles that no row's mask touches"
    assert any(hi < sk and hi % 64 != 0 for _, _, hi in rows), "a tile cut by the causal diagonal"
    if ep == "partial":
        assert case["splits"] == 3
        for blk in blocks:
            assert [hi - lo for lo, hi in blk["parts"]] in ([4, 4, 4], [4, 4, 3])
            assert all(lo < hi and (lo + 1) * 64 <= sk for lo, hi in blk["parts"]), "every part owns a full tile"
        for n in lens:  # ... and no part of any entry is empty
            assert all(lo < hi for blk in U.replay(sq, n, g, block, causal=True, splits=3) for lo, hi in blk["parts"])
    else:
        assert case["splits"] == 1


@pytest.mark.parametrize("form,ep,case", [(f, ep, c) for f, ep, dt, c in CASES if dt == "bf16"],
                         ids=[i for i, (_, _, dt, _) in zip(IDS, CASES) if dt == "bf16"])
def test_universe_case_geometry(form, ep, case):
    _check_geometry(form, ep, case)


def test_geometry_check_notices_a_broken_case():
    """The geometry conditions discriminate: a fill level that is a multiple of 64, equal fill levels, and packed rows that are
    a multiple of the row block each fail."""
    form = "kv8_fwd_kernel D=128 waves=4"
    good = U.FORMS[form]["partial"]
    _check_geometry(form, "partial", good)
    for broken in (dict(good, lens=(704, 651)), dict(good, lens=(715, 715)), dict(good, sq=128), dict(good, h=8)):
        with pytest.raises(AssertionError):
            _check_geometry(form, "partial", broken)


def test_softcap_cases_leave_the_linear_part_of_the_tanh():
    """Descales of 0.5 .. 16 make the factor in front of the tanh differ per (batch, kv head).  Unit-variance q / k / v / qv
    give a descaled, scaled score of standard deviation k_descale (kv8) and sqrt((kd^2 d + vd^2 d_v) / (d + d_v)) (qv8): at
    least one (batch, kv head) reaches SOFTCAP / 2 (tanh(0.5) is 8% under its argument), and the factors differ."""
    from test_kv8_kvcache_gpu import _descales
    for form, by_ep in U.FORMS.items():
        if " SOFTCAP" not in form:
            continue
        for case in by_ep.values():
            assert case["softcap"] == U.SOFTCAP
            kd, vd = _descales(case["b"], case["hk"], 0), _descales(case["b"], case["hk"], 3)
            if case["kernel"] == "kv8":
                std = kd
            else:
                std = ((kd ** 2 * case["d"] + vd ** 2 * case["dv"]) / (case["d"] + case["dv"])).sqrt()
            assert std.max().item() >= U.SOFTCAP / 2 and len(set(std.flatten().tolist())) == case["b"] * case["hk"], std


# ---- the edge set of the partial epilogue ----------------------------------------------------------------------------------------
def test_edge_set_runs_both_kernels_and_fp16_where_asked():
    got = {(name, kernel, dt) for name, kernel, dt, _ in U.edge_cases()}
    for name in U.EDGES:
        assert {(name, "kv8", "bf16"), (name, "qv8", "bf16")} <= got
    for name in ("ragged-dense", "ragged-page16", "masked-part"):
        assert {(name, "kv8", "fp16"), (name, "qv8", "fp16")} <= got
    for name, kernel, _, kw in U.edge_cases():  # every case really splits three ways: the capacity has at least 3 key tiles
        assert kw.get("cap", 320) // 64 >= 3


@pytest.mark.parametrize("kernel", ["kv8", "qv8"])
def test_edge_ragged_queries(kernel):
    kw = U.EDGES["ragged-dense"][kernel == "qv8"]
    cu, used = kw["cu_q"], kw["seqused_q"]
    ranges = [cu[i + 1] - cu[i] for i in range(kw["b"])]
    assert 0 in ranges, "a sequence without queries"
    assert any(u < r for u, r in zip(used, ranges)) and all(u <= r for u, r in zip(used, ranges)), "seqused_q shorter than a range"
    assert U.EDGES["ragged-page16"][kernel == "qv8"]["page"] == 16


@pytest.mark.parametrize("kernel", ["kv8", "qv8"])
def test_edge_paged_fill_levels(kernel):
    for name, page in (("page64", 64), ("page16", 16)):
        kw = U.EDGES[name][kernel == "qv8"]
        assert kw["page"] == page and kw["cap"] % page == 0
        assert any(n % page == 0 for n in kw["lens"]) and any(n % page != 0 and n > page for n in kw["lens"])
    kw = U.EDGES["cache_batch_idx"][kernel == "qv8"]
    assert len(set(kw["batch_idx"])) < len(kw["batch_idx"]) and "page" not in kw
    assert "page" not in U.EDGES["leftpad_k"][kernel == "qv8"]


@pytest.mark.parametrize("kernel", ["kv8", "qv8"])
def test_edge_part_emptied_by_the_mask(kernel):
    """One row block whose three parts own one or more tiles each, all inside the fill level: some of its rows see no key of the
    first part, others none of the last, and every row sees keys -- so the `-inf` branch of the epilogue (`empty && lim_lo <
    lim_hi`) is taken because of the mask, not the fill level."""
    kw = U.EDGES["masked-part"][kernel == "qv8"]
    (blocks,) = U.edge_geometry(kernel, kw)
    sk = kw["lens"][0]
    blk = blocks[0]
    assert all(lo < hi and lo * 64 < sk for lo, hi in blk["parts"]), blk["parts"]
    assert all(lo < hi for b in blocks for _, lo, hi in b["rows"]), "every row sees keys"
    first, last = blk["parts"][0], blk["parts"][-1]
    no_first = [r for r in blk["rows"] if not U.sees(r, first)]
    no_last = [r for r in blk["rows"] if not U.sees(r, last)]
    assert any(U.sees(r, last) for r in no_first), "a row that sees keys of the last part and none of the first"
    assert any(U.sees(r, first) for r in no_last), "a row that sees keys of the first part and none of the last"


@pytest.mark.parametrize("kernel", ["kv8", "qv8"])
def test_edge_keyless_rows_share_a_block_with_rows_that_see_keys(kernel):
    kw = U.EDGES["keyless-rows"][kernel == "qv8"]
    assert kw["sq"] > min(kw["lens"])
    shared = False
    for blocks in U.edge_geometry(kernel, kw):
        for blk in blocks:
            keyless = [r for r in blk["rows"] if r[1] >= r[2]]
            if keyless and len(keyless) < len(blk["rows"]):
                shared = True
                assert blk["parts"][0][0] < blk["parts"][0][1], "the block's tile is processed"
                assert not any(U.sees(r, p) for r in keyless for p in blk["parts"])
    assert shared


@pytest.mark.parametrize("kernel", ["kv8", "qv8"])
def test_edge_several_row_blocks(kernel):
    kw = U.EDGES["row-blocks"][kernel == "qv8"]
    g = kw["h"] // kw["hk"]
    assert (kw["sq"], g, kw["sq"] * g) == ((130, 4, 520) if kernel == "kv8" else (40, 4, 160))
    assert kernel == "qv8" or kw["d"] == 64
    assert all(len(blocks) == 5 for blocks in U.edge_geometry(kernel, kw)) and 250 <= max(kw["lens"]) <= 320
