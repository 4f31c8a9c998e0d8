"""The ctypes binding against the header: capi.SIGNATURES row by row, capi.bind, poa._entry, the shared default_params body and
the one PAF ingest.  CPU only: the libraries load without a device."""
import ctypes as C
import gzip
import io
import os
import re
import types

import numpy as np
import pytest

from vechat_amd import align, capi, cluster, overlap, poa, scrub

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# declared in the header, never called from Python: vc_io_load feeds the window builder through them inside the library
NOT_CALLED_FROM_PYTHON = {"vc_wb_add_sequence_view": "the copy-free form of vc_wb_add_sequence, for vc_io_load's record buffers",
                          "vc_wb_add_overlaps": "the batched form of vc_wb_add_overlap, for vc_io_load's overlap set"}


def header_prototypes():
    """[(name, parameter count)] of every vc_* prototype of the header, in its order"""
    text = open(os.path.join(ROOT, "include", "vechat_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    out = []
    for name, params in re.findall(r"\b(vc_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", text):
        params = " ".join(params.split())
        out.append((name, 0 if params in ("", "void") else params.count(",") + 1))
    return out


def test_the_table_matches_the_header():
    protos = header_prototypes()
    assert len(protos) == len({n for n, _ in protos}) > 100                       # every name once; the parser found the header
    assert dict(protos)["vc_has_experiments"] == 0 and dict(protos)["vc_poa_run_from"] == 10 and dict(protos)["vc_weight_lut"] == 1
    assert not set(NOT_CALLED_FROM_PYTHON) & set(capi.SIGNATURES)
    assert {n for n, _ in protos} == set(capi.SIGNATURES) | set(NOT_CALLED_FROM_PYTHON)
    assert [n for n, _ in protos if n in capi.SIGNATURES] == list(capi.SIGNATURES)          # rows in the order of the header
    wrong = {n: (k, len(capi.SIGNATURES[n][1])) for n, k in protos if n in capi.SIGNATURES and len(capi.SIGNATURES[n][1]) != k}
    assert not wrong, wrong
    for name, (restype, argtypes) in capi.SIGNATURES.items():
        assert isinstance(argtypes, list), name                                      # an entry without arguments has [], not None


def test_the_table_matches_the_loaded_libraries(built):
    hip, host = capi.load_hip(), capi.load_host()
    assert capi.HOST_ENTRIES[0] == "vc_rank_layers" and capi.HOST_ENTRIES[-1] == "vc_io_load" and "vc_synth_generate" in capi.HOST_ENTRIES
    assert not any(n.startswith(("vc_poa", "vc_align", "vc_large", "vc_overlap", "vc_scrub", "vc_cluster")) for n in capi.HOST_ENTRIES)
    for lib, names in ((hip, capi.SIGNATURES), (host, capi.HOST_ENTRIES)):
        for name in names:
            restype, argtypes = capi.SIGNATURES[name]
            fn = getattr(lib, name)
            assert fn.restype is restype and list(fn.argtypes) == argtypes, name
    with pytest.raises(TypeError):                                                   # typed: a call that leaves an argument out is refused
        hip.vc_poa_run_gaps(None, None)


def test_the_structures_stay_importable_from_their_modules():
    for module, names in ((overlap, ("VcOverlapSeqs", "VcOverlapParams", "VcOverlapOut", "VcOverlapSketchOut")),
                          (scrub, ("VcScrubParams", "VcScrubIn", "VcScrubOut")),
                          (cluster, ("VcClusterParams", "VcClusterIn", "VcClusterOut")), (align, ("VcAlignBatch",))):
        for name in names:
            assert getattr(module, name) is getattr(capi, name), name
    assert overlap.PARAMS == ("k", "w", "max_occ", "max_gap", "bandwidth", "lookback", "min_chain_score", "min_anchors", "min_overlap",
                              "drop_internal", "same_set")
    assert scrub.PARAMS == ("coverage", "max_bad_permille", "min_piece")
    assert cluster.PARAMS == ("min_overlap", "min_cover_permille", "cover_both", "min_identity_permille", "min_size", "by_size", "longest_first")
    assert C.sizeof(capi.VcOverlapParams) == 48 and C.sizeof(capi.VcScrubParams) == 16 and C.sizeof(capi.VcClusterParams) == 32
    assert scrub.PRESETS is overlap.PRESETS and cluster.PRESETS is overlap.PRESETS


class _Fn:
    """what a library object hands out for a symbol: something that takes restype and argtypes"""
    restype = argtypes = "untouched"


SENTENCE = "this libvechat_hip.so has no vc_poa_run_spans: it was built before the entry point existed; rebuild it"


def test_bind_and_entry_on_a_library_that_lacks_symbols():
    names = ("vc_poa_run_gaps", "vc_poa_run_spans", "vc_poa_run_weighted", "vc_poa_last_error")
    old = types.SimpleNamespace(vc_poa_run_gaps=_Fn(), vc_poa_last_error=_Fn(), vc_poa_run=_Fn())
    assert capi.bind(old, names, optional=True) is old
    for name in ("vc_poa_run_gaps", "vc_poa_last_error"):
        assert (getattr(old, name).restype, getattr(old, name).argtypes) == capi.SIGNATURES[name]
    assert old.vc_poa_run.argtypes == "untouched" and not hasattr(old, "vc_poa_run_spans")      # only the named ones; nothing made up
    with pytest.raises(AttributeError) as e:
        capi.bind(old, names)
    assert "vc_poa_run_spans" in str(e.value) and "vc_poa_run_weighted" not in str(e.value)     # the first one missing
    with pytest.raises(AttributeError, match="vc_create"):
        capi.bind(old)                                                                           # names=None: every row
    assert poa._entry(old, "vc_poa_run_gaps") is old.vc_poa_run_gaps
    with pytest.raises(poa.PoaError) as e:
        poa._entry(old, "vc_poa_run_spans")
    assert str(e.value) == SENTENCE
    with pytest.raises(poa.PoaError) as e:                       # and through a call: the request for spans finds the same sentence
        poa.poa_consensus([["ACGT", "ACGT"]], spans=[[None, (0, 3)]], lib=old)
    assert str(e.value) == SENTENCE


@pytest.mark.parametrize("module, what, field", [(overlap, "overlap", "max_gap"), (scrub, "scrub", "min_piece"), (cluster, "cluster", "min_size")])
def test_default_params_are_the_c_defaults_with_keywords_on_top(built, module, what, field):
    lib = capi.load_hip()
    struct = getattr(capi, "Vc%sParams" % what.capitalize())
    want = struct()
    getattr(lib, "vc_%s_default_params" % what)(C.byref(want))
    fields = [f for f, _ in struct._fields_]
    assert fields == ["device"] + list(module.PARAMS)
    got = module.default_params(lib)
    assert isinstance(got, struct) and [getattr(got, f) for f in fields] == [getattr(want, f) for f in fields]
    assert any(getattr(want, f) for f in fields)                                     # the C function did write
    got = module.default_params(lib, device=3, **{field: 77})
    assert [getattr(got, f) for f in fields] == [3 if f == "device" else 77 if f == field else getattr(want, f) for f in fields]
    with pytest.raises(TypeError) as e:
        module.default_params(lib, no_such_field=1)
    assert str(e.value) == f"unknown {what} parameter 'no_such_field'"


PAF = ("r1\t100\t5\t95\t-\tr0\t120\t10\t110\t80\t100\t255\tcg:Z:90M\n"
       "r0\t120\t0\t50\t+\tr2\t60\t10\t60\t45\t50\t255\n"
       "\n"
       "r2\t60\t0\t60\t+\tr1\t100\t40\t100\t58\t61\t255\n"
       "r0\t120\t60\t120\t-\tr2\t60\t0\t60\t55\t60\t0\n")
NAMES = ["r0", "r1", "r2"]
# what the code before the shared ingest gave for PAF: cluster.records_from_paf, and the interval array of scrub.main --paf
RECORDS = dict(q_id=[1, 0, 2, 0], t_id=[0, 2, 1, 2], strand=[1, 0, 0, 1], q_begin=[5, 0, 0, 60], q_end=[95, 50, 60, 120],
               t_begin=[10, 10, 40, 0], t_end=[110, 60, 100, 60], matches=[80, 45, 58, 55], block=[100, 50, 61, 60])
INTERVALS = [[1, 5, 95], [0, 10, 110], [0, 0, 50], [2, 10, 60], [2, 0, 60], [1, 40, 100], [0, 60, 120], [2, 0, 60]]


@pytest.fixture
def paf_files(tmp_path):
    (tmp_path / "o.paf").write_text(PAF)
    with gzip.open(tmp_path / "o.paf.gz", "wt") as f:
        f.write(PAF)
    (tmp_path / "reads.fa").write_text(">r0 first\n" + "A" * 120 + "\n>r1\n" + "C" * 100 + "\n>r2\n" + "G" * 60 + "\n")
    return tmp_path


def scrub_intervals(monkeypatch, argv):
    """the interval array scrub.main hands to scrub() for these arguments; the device call is replaced by one that keeps it"""
    seen = {}

    def keep(reads, intervals, **kw):
        seen["intervals"] = intervals
        return [], {"pc_read": []}

    monkeypatch.setattr(scrub, "scrub", keep)
    assert scrub.main(argv, out=io.StringIO()) == 0
    return seen["intervals"]


@pytest.mark.parametrize("name", ["o.paf", "o.paf.gz"])
def test_one_paf_ingest_serves_cluster_and_scrub(paf_files, monkeypatch, name):
    path = str(paf_files / name)
    assert tuple(RECORDS) == tuple(f for f, _ in cluster.RECORD_FIELDS)
    for rec in (overlap.records_from_paf(path, NAMES, "is unknown"), cluster.records_from_paf(path, NAMES)):
        assert list(rec) == list(RECORDS)
        for f in RECORDS:
            assert rec[f].dtype == np.int64 and rec[f].tolist() == RECORDS[f], f
    iv = scrub_intervals(monkeypatch, ["--paf", path, str(paf_files / "reads.fa")])
    assert iv.dtype == np.int64 and iv.shape == (8, 3) and iv.tolist() == INTERVALS


def test_a_paf_line_that_names_an_unknown_read(paf_files, monkeypatch):
    path, reads = str(paf_files / "o.paf"), str(paf_files / "reads.fa")
    with open(path, "a") as f:
        f.write("r0\t120\t0\t50\t+\tr9\t60\t10\t60\t45\t50\t255\n")
    with pytest.raises(ValueError) as e:
        overlap.records_from_paf(path, NAMES, "is unknown")
    assert str(e.value) == f"{path}: 'r9' is unknown"
    with pytest.raises(ValueError) as e:
        cluster.records_from_paf(path, NAMES)
    assert str(e.value) == f"{path}: 'r9' is not a read of the input"
    with pytest.raises(ValueError) as e:
        scrub_intervals(monkeypatch, ["--paf", path, reads])
    assert str(e.value) == f"{path}: 'r9' is not a read of {reads}"
    (paf_files / "bad.paf").write_text("r0\t120\t50\t40\t+\tr1\t100\t0\t10\t5\t10\t255\n")       # begin > end: the reader's own refusal
    with pytest.raises(ValueError, match="malformed PAF record"):
        cluster.records_from_paf(str(paf_files / "bad.paf"), NAMES)
    (paf_files / "none.paf").write_text("\n")
    assert {f: v.tolist() for f, v in cluster.records_from_paf(str(paf_files / "none.paf"), NAMES).items()} == {f: [] for f in RECORDS}
