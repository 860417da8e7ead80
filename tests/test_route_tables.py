"""The tables of tests/test_gpu_routes.py against the sources, without a GPU: every option of options.h has a row, the ledgers name
as many instantiations as the launch tables hold, and every ledger entry routes -- in the library's own host code -- to the kernel
it names."""
import ctypes as C
import glob
import os
import re

from tests import route_cases as R
from tests import test_gpu_routes as G
from vinet_amd import _lib as L

CSRC = os.path.join(G.ROOT, "vinet_amd", "csrc")


def _src(name):
    """the file without comments and macro definitions (continuation lines included): what is left instantiates"""
    out, in_macro = [], False
    for l in open(os.path.join(CSRC, name)).read().split("\n"):
        macro = in_macro or l.lstrip().startswith("#define")
        in_macro = macro and l.rstrip().endswith("\\")
        if not macro and not l.lstrip().startswith("//"):
            out.append(l)
    return "\n".join(out)


def missing_option_rows(header, rows):
    """options of `header` without a row, rows without an option, rows that say nothing"""
    names = set(R.option_defaults(header))
    bad = sorted(names - set(rows)) + sorted(set(rows) - names)
    for n, r in rows.items():
        if r["kind"] == "exempt" and len(r["reason"]) < 5:
            bad.append(n + ": exemption without a reason")
        if r["kind"] == "sweep" and not (r["values"] and r["cases"]):
            bad.append(n + ": sweep without values or cases")
    return bad


def test_every_option_has_a_row():
    assert len(R.option_defaults(G.OPTIONS_H)) == len(re.findall(r"^\s*VN_OPT\(\w", open(G.OPTIONS_H).read(), flags=re.M)) == 49
    assert not missing_option_rows(G.OPTIONS_H, G.OPTION_ROWS)


def test_a_new_option_without_a_row_fails(tmp_path):
    txt = open(G.OPTIONS_H).read().replace('  VN_OPT(dma3,', '  VN_OPT(brand_new,   3, "an option nobody swept") \\\n  VN_OPT(dma3,')
    h = tmp_path / "options.h"
    h.write_text(txt)
    assert missing_option_rows(str(h), G.OPTION_ROWS) == ["brand_new"]


def test_sweep_values_differ_from_the_defaults_and_named_tests_exist():
    defs = "\n".join(open(f).read() for f in glob.glob(os.path.join(G.ROOT, "tests", "test_gpu_*.py")))
    for n, r in G.OPTION_ROWS.items():
        if r.get("values"):
            assert G.OPT_DEFAULTS[n] not in r["values"], n
        if r.get("test"):
            assert re.search(r"^def %s\(" % r["test"], defs, flags=re.M), "%s: no test %s" % (n, r["test"])
        if r["kind"] == "sweep":
            for k in list(r["base"]) + [n]:
                assert k in G.OPT_DEFAULTS, k


def test_ledger_counts_match_the_launch_tables():
    bf, f32, bnb = _src("conv_bf16.hip"), _src("conv_f32.hip"), _src("conv_bnb.hip")
    cfg = r"launch_conv_\w*cfg<"
    counts = {"conv_bf16.hip": len(re.findall(r"\bCASE\(\d", bf)) + 2 * len(re.findall(r"\bDMA_CASE\(\d", bf)) + len(re.findall(cfg, bf)),
              "conv_f32.hip": 2 * len(re.findall(r"\bCASE\(\d", f32)) + len(re.findall(cfg, f32)),
              "conv_bnb.hip": len(re.findall(r"\bDMA_BNB_CASE\(\d", bnb)) + len(re.findall(cfg, bnb))}
    assert counts == R.CONV_INSTANTIATION_COUNTS
    assert len(set(R.CONV_INSTANTIATIONS_RUN)) == len(R.CONV_INSTANTIATIONS_RUN)
    assert len(R.CONV_INSTANTIATIONS_RUN) + len(R.CONV_INSTANTIATIONS_NOT_RUN) == sum(counts.values()) == 107
    ledger = {e.name + (" [bnb]" if "[bnb]" in e.key else "") for e in G.CONV_LEDGER}
    assert ledger == set(R.CONV_INSTANTIATIONS_RUN), ledger ^ set(R.CONV_INSTANTIATIONS_RUN)
    wg = _src("wgrad_dma.hip")
    assert len(re.findall(r"\bWG\(\d", wg)) == 6 and len(re.findall(r"launch_wg<64, 32, 7", wg)) == 1
    assert {e.name for e in G.WGRAD_LEDGER} == set(R.WGRAD_NAMES_RUN)
    for W in (24, 48, 32, 64, 96):      # both forms of the row-streaming kernel wherever the four-wave one exists
        assert {"conv_wgrad_rs_kernel<W%d,4w>" % W, "conv_wgrad_rs_kernel<W%d,8w>" % W} <= {e.name for e in G.WGRAD_LEDGER}
    assert len([n for n in R.WGRAD_NAMES_RUN + list(R.WGRAD_NAMES_NOT_RUN) if "wgrad_dma" in n]) == 2 * 6 + 1


def test_every_ledger_entry_routes_to_its_name_on_the_host():
    lib = L.load()
    for e in G.CONV_LEDGER:
        with R.options(lib, e.opts, G.OPT_DEFAULTS):
            d = R.stem_desc(e.dt) if e.runner == "stem" else R.conv_desc(e.case, e.dt, e.cdt)
            assert R.conv_name(lib, d) == e.name, (e.key, R.conv_name(lib, d))
            if "[bnb]" in e.key:
                assert lib.vinet_conv3d_bn_bwd_stats_rows(C.byref(d)) > 0, e.key
            if "[natural" in e.key:
                assert not e.opts
    for e in G.WGRAD_LEDGER:
        with R.options(lib, e.opts, G.OPT_DEFAULTS):
            assert R.wgrad_name(lib, R.wgrad_desc(e.case, e.dt, e.cdt)) == e.name, (e.key, R.wgrad_name(lib, R.wgrad_desc(e.case, e.dt, e.cdt)))
    # the natural route of the two 256-row tiles of the large-M inference path: only the ladder switches (and n128_kmax for the wide one) set
    big = {e.name: e for e in G.CONV_LEDGER if e.case and e.case[1] == G.BIG and "[" not in e.key}
    assert set(big["conv_dma_kernel<4,4,4,1,3,plain>"].opts) == set(G.LADDER) and set(big["conv_dma_kernel<4,8,4,1,3,plain>"].opts) == set(G.LADDER) | {"n128_kmax"}


def test_sweep_rows_change_the_route_they_claim_on_the_host():
    lib = L.load()
    for n, r in G.OPTION_ROWS.items():
        if r["kind"] != "sweep" or r["claim"] is None:
            continue
        for case, dt, cdt in r["cases"]:
            if G._is_wgrad(case):      # (the weight-gradient rows claim a name change: checked where they run)
                continue
            def info(o):
                with R.options(lib, o, G.OPT_DEFAULTS):
                    d = R.conv_desc(case, dt, cdt)
                    return (R.conv_name(lib, d), lib.vinet_conv3d_tile_m(C.byref(d)), lib.vinet_conv3d_stats_rows(C.byref(d)), lib.vinet_conv3d_splitk_bytes(C.byref(d)))
            base = info(r["base"])
            changed = [info(dict(r["base"], **{n: v})) != base for v in r["values"]]
            if "@" in r["claim"]:
                flip = r["values"].index(int(r["claim"].split("@")[1]))
                assert changed == [j == flip for j in range(len(changed))], (n, case[0], changed)
            elif r["claim"] == "any":
                assert any(changed), (n, case[0])
            else:
                assert all(changed), (n, case[0], changed)


def test_n64_kmax_flips_the_tile_on_the_host():
    """n64_kmax is gated by M >= 2^20 rows: no launch of that size in this suite, the route alone"""
    lib = L.load()
    case = ("n64_m2p20", (8, 8, 128, 128), 64, 64, (1, 3, 3), (1, 1, 1), (0, 1, 1), {})      # 18 K steps of 32
    names = {}
    for v in (17, 18, G.OPT_DEFAULTS["n64_kmax"]):
        with R.options(lib, dict(G.LADDER, n64_kmax=v), G.OPT_DEFAULTS):
            names[v] = R.conv_name(lib, R.conv_desc(case, G.BF16))
    assert names[17] == "conv_dma_kernel<4,4,4,1,3,plain>" and names[18] == names[64] == "conv_dma_kernel<4,2,2,2,3,plain>", names


def test_wgrad_name_tells_the_row_streaming_forms_apart():
    lib = L.load()
    for W, four in ((24, True), (48, True), (32, True), (64, True), (96, True), (128, False), (160, False), (192, False)):
        case = ("rs", (1, 2, 4, W), 64, 64, (1, 3, 3), (1, 1, 1), (0, 1, 1), False, dict(tline=4))
        with R.options(lib, dict(wgrad_rs=2), G.OPT_DEFAULTS):
            assert R.wgrad_name(lib, R.wgrad_desc(case, G.BF16)) == "conv_wgrad_rs_kernel<W%d,%s>" % (W, "4w" if four else "8w")
            with R.options(lib, dict(wgrad_rs4=0), G.OPT_DEFAULTS):
                assert R.wgrad_name(lib, R.wgrad_desc(case, G.BF16)) == "conv_wgrad_rs_kernel<W%d,8w>" % W


def test_tperm_weight_gradient_cases_take_the_permuted_order():
    """wgrad_pp.hip:436 / wgrad_dma.hip:374: the t-fastest K-tile order needs To > 1 and Ho x Wo % 64 (ping-pong) / % 32 (LDS-DMA) == 0"""
    lib = L.load()
    seen = set()
    for c in G.OPTION_ROWS["tperm"]["cases"]:
        if not G._is_wgrad(c[0]):
            continue
        with R.options(lib, dict(c[3], tperm=1), G.OPT_DEFAULTS):
            d = R.wgrad_desc(c[0], c[1])
            name = R.wgrad_name(lib, d)
        assert d.dy.T > 1 and (d.dy.H * d.dy.W) % (64 if "_pp_" in name else 32) == 0, c[0][0]
        seen.add(name.split("<")[0] + ("<%d>" % c[3]["wgrad_pp"] if "_pp_" in name else ""))
    assert seen == {"conv_wgrad_pp_kernel<3>", "conv_wgrad_pp_kernel<4>", "conv_wgrad_dma_kernel"}, seen


def test_pool_table_names_every_instantiation_of_pool_hip():
    src = _src("pool.hip")
    typed, plain = re.findall(r"hipLaunchKernelGGL\((\w+)<T>", src), re.findall(r"hipLaunchKernelGGL\((\w+),", src)
    assert len(typed) == len(set(typed)) == 11 and len(plain) == len(set(plain)) == 3      # DISPATCH_T: two dtypes per typed site
    inst = {"%s<%s>" % (k, t) for k in typed for t in ("f32", "bf16")} | set(plain)
    assert len(inst) == 25 and len([n for n in inst if "_bwd" in n]) == 13
    assert ({c[8] for c in R.POOL_TABLE} | {c[9] for c in R.POOL_TABLE}) - {None} == inst      # (None: a rejected call)
    assert len({c[0] for c in R.POOL_TABLE}) == len(R.POOL_TABLE)
    for opt, values in (("pool_lds", {0, 1, 2}), ("pool_pk", {0, 1}), ("pool_twalk", {0, 1, 2, 3}), ("pool_blk", {0, 1})):      # every documented value
        assert {c[7].get(opt, G.OPT_DEFAULTS[opt]) for c in R.POOL_TABLE} == values, opt


def test_pool_table_routes_on_the_host():
    lib = L.load()
    for key, ksp, dt, dims, chan, pre, am, opts, fwd, bwd in R.POOL_TABLE:
        with R.options(lib, opts, G.OPT_DEFAULTS):
            assert R.pool_names(lib, *R.pool_args(ksp, dt, dims, chan, pre, am)) == (fwd, bwd), key
