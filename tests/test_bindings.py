"""The Python binding against include/kmer_spans.h: every prototype, struct
and integer constant of the header compared with the hand-written table,
ctypes.Structure mirrors and constants of kmer_spans_amd/_lib.py, and the order
in which the api.region_* wrappers raise their argument errors.  CPU only: the
built library is needed for hasattr alone, no call reaches a device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from kmer_spans_amd import _lib, api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SCALARS = {"int32_t": "i32", "ks_status": "i32", "int64_t": "i64", "double": "f64", "size_t": "size"}

# the header's struct typedefs and their mirrors
STRUCTS = {
    "ks_regions": _lib.Regions, "ks_dev_seqs": _lib.DevSeqs, "ks_table_info": _lib.TableInfo,
    "ks_table_props": _lib.TableProps, "ks_scan_stats": _lib.ScanStats, "ks_seq_index_info": _lib.SeqIndexInfo,
    "ks_fasta": _lib.Fasta, "ks_count_file": _lib.CountFile, "ks_kmer_file_info": _lib.KmerFileInfo,
    "ks_spectra_stats": _lib.SpectraStats, "ks_dist_stats": _lib.DistStats, "ks_hclust_stats": _lib.HclustStats,
    "ks_nj_stats": _lib.NjStats, "ks_silhouette_stats": _lib.SilhouetteStats, "ks_pca_stats": _lib.PcaStats,
    "ks_kmeans_result": _lib.KmeansResult, "ks_kmeans_stats": _lib.KmeansStats, "ks_seed_result": _lib.SeedResult,
    "ks_seed_stats": _lib.SeedStats, "ks_knn_stats": _lib.KnnStats,
}


# ------------------------------------------------------------ the header, parsed

def header_code() -> str:
    """include/kmer_spans.h without its comments."""
    with open(os.path.join(ROOT, "include", "kmer_spans.h")) as f:
        text = f.read()
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))


def c_kind(decl: str) -> str:
    """pointer (any *), or the scalar type named in a parameter, field or return type."""
    if "*" in decl:
        return "ptr"
    names = [SCALARS[w] for w in re.findall(r"\w+", decl) if w in SCALARS]
    assert len(names) == 1, f"no single known scalar type in {decl!r}"
    return names[0]


def header_prototypes() -> dict:
    """name -> ([kind of every parameter], kind of the return value) of every
    `ret ks_name(args);` of the header, across lines."""
    code = re.sub(r"typedef\s+struct\s+\w*\s*\{.*?\}\s*\w+\s*;", "", header_code(), flags=re.S)
    code = "\n".join(ln for ln in code.split("\n") if not ln.lstrip().startswith("#") and 'extern "C"' not in ln)
    out = {}
    for stmt in code.split(";"):
        if "(" not in stmt:
            continue
        m = re.fullmatch(r"\s*([\w\s\*]+?)\s*\b(ks_\w+)\s*\((.*)\)\s*", stmt, flags=re.S)
        assert m, f"a statement with parentheses that is no prototype: {stmt!r}"
        ret, name, args = m.group(1).strip(), m.group(2), m.group(3).strip()
        assert name not in out, name
        params = [] if args == "void" else [c_kind(a) for a in args.split(",")]
        out[name] = (params, "void" if ret == "void" else c_kind(ret))
    return out


def header_structs() -> dict:
    """name -> [(field, kind)] in order, of every `typedef struct { ... } ks_*;`.
    kind: ptr, a scalar kind, ("char", n) for a char array, ("struct", name)."""
    out = {}
    for body, name in re.findall(r"typedef\s+struct\s+\w*\s*\{(.*?)\}\s*(ks_\w+)\s*;", header_code(), flags=re.S):
        fields = []
        for decl in body.split(";"):
            decl = decl.strip()
            if not decl:
                continue
            m = re.fullmatch(r"(?:const\s+)?(\w+)\s+(?:const\s+)?(.+)", decl, flags=re.S)
            assert m, decl
            base = m.group(1)
            for d in m.group(2).split(","):
                dm = re.fullmatch(r"\s*(\**)\s*(?:const\s+)?(\w+)\s*(?:\[(\d+)\])?\s*", d)
                assert dm, (name, decl)
                stars, field, arr = dm.groups()
                if stars:
                    kind = "ptr"
                elif arr:
                    assert base == "char", (name, decl)
                    kind = ("char", int(arr))
                elif base in SCALARS:
                    kind = SCALARS[base]
                else:
                    kind = ("struct", base)
                fields.append((field, kind))
        out[name] = fields
    return out


def header_constants() -> dict:
    """Every `#define KS_NAME integer` of the header."""
    return {n: int(v, 0) for n, v in re.findall(r"^\s*#define\s+(KS_\w+)\s+(-?(?:0x[0-9a-fA-F]+|\d+))\s*$",
                                                header_code(), flags=re.M)}


def ctypes_kind(t):
    if t is None:
        return "void"
    if t in (C.c_void_p, C.c_char_p) or issubclass(t, C._Pointer):
        return "ptr"
    if issubclass(t, C.Array):
        assert t._type_ is C.c_char
        return ("char", t._length_)
    if issubclass(t, C.Structure):
        return ("struct", {v: k for k, v in STRUCTS.items()}[t])
    return {C.c_int32: "i32", C.c_int64: "i64", C.c_double: "f64", C.c_size_t: "size"}[t]


def prototype_mismatches(table, protos) -> list:
    bad = []
    for name, (params, ret) in protos.items():
        if name not in table:
            bad.append((name, "not in the table"))
            continue
        args, res = table[name]
        got = ([ctypes_kind(a) for a in args], ctypes_kind(res))
        if got != (params, ret):
            bad.append((name, "table", got, "header", (params, ret)))
    return bad


def struct_mismatches(structs, parsed) -> list:
    bad = []
    for name, fields in parsed.items():
        got = [(f, ctypes_kind(t)) for f, t in structs[name]._fields_]
        if got != fields:
            bad.append((name, "mirror", got, "header", fields))
    return bad


# ---------------------------------------------------------------- prototypes

def test_parser_reads_the_declarations_it_should():
    """The parser itself, on the shapes the header uses."""
    protos = header_prototypes()
    assert protos["ks_last_error"] == ([], "ptr") and protos["ks_release_cache"] == ([], "void")
    assert protos["ks_kmer_seq"] == (["i32", "ptr", "size"], "i32")
    assert protos["ks_table_escape_fraction"] == (["ptr"], "f64")
    assert protos["ks_shard_plan"] == (["ptr", "ptr", "i32", "i32", "ptr", "i64"], "i64")
    assert len(protos["ks_silhouette_dev"][0]) == 17
    structs = header_structs()
    assert structs["ks_table_info"][:4] == [("k", "i32"), ("compressed", "i32"), ("positions_per_read", "i32"),
                                            ("code_bits", "i32")]
    assert structs["ks_fasta"][:2] == [("seqs", ("struct", "ks_dev_seqs")), ("names", "ptr")]
    assert structs["ks_kmer_file_info"][-2:] == [("out_path", ("char", 4096)), ("message", ("char", 512))]
    assert structs["ks_count_file"][-1] == ("counts", "ptr")


def test_every_prototype_matches_the_table():
    protos = header_prototypes()
    assert len(protos) == 92
    assert _lib.EXPORTS == list(_lib.SIGNATURES) and set(_lib.EXPORTS) == set(protos), \
        set(_lib.EXPORTS) ^ set(protos)
    assert prototype_mismatches(_lib.SIGNATURES, protos) == []
    L = _lib.load()
    for name in protos:
        assert hasattr(L, name), name
        assert list(getattr(L, name).argtypes) == _lib.SIGNATURES[name][0], name


# ------------------------------------------------------------------- structs

def test_every_struct_matches_its_mirror():
    parsed = header_structs()
    assert set(parsed) == set(STRUCTS) and len(parsed) == 20
    mirrors = {v for v in vars(_lib).values()
               if isinstance(v, type) and issubclass(v, C.Structure) and hasattr(v, "_fields_")}
    assert mirrors == set(STRUCTS.values()), mirrors ^ set(STRUCTS.values())
    assert struct_mismatches(STRUCTS, parsed) == []


def test_stats_structures_give_every_field():
    stats = [c for c in STRUCTS.values() if issubclass(c, _lib.Stats)]
    assert len(stats) == 12
    for cls in stats + [_lib.SeqIndexInfo]:
        names = [f for f, _ in cls._fields_]
        d = cls().as_dict()
        assert list(d) == names and all(v == 0 for v in d.values()), cls.__name__
    inf = _lib.SeqIndexInfo(builds=3, hits=2**40)
    assert inf.as_dict(_lib.SeqIndexInfo.INDEX_FIELDS) == {"builds": 3, "hits": 2**40, "layout_builds": 0,
                                                           "guard_failures": 0}
    assert all(type(v) is int for v in inf.as_dict().values())


# ----------------------------------------------------------------- constants

def test_constants_match_the_header():
    consts = header_constants()
    assert consts["KS_OK"] == 0 and consts["KS_DIST_MAX_NCOL"] == 4096 and consts["KS_TABLE_PART_APPROX"] == 8
    mirrored = {n: v for n, v in vars(_lib).items() if n.startswith("KS_") and isinstance(v, int)}
    assert {"KS_OK", "KS_MAX_K", "KS_SPECTRA_MAX_Q", "KS_NJ_NO_COMPACT", "KS_KNN_MAX_K"} <= set(mirrored)
    for name, value in mirrored.items():
        assert consts[name] == value, name
    assert _lib.HCLUST_METHODS == {m: consts["KS_HCLUST_" + m.upper()] for m in ("complete", "single", "average")}
    assert _lib.SEED_METHODS == {"maximin": consts["KS_SEED_MAXIMIN"], "kmeans++": consts["KS_SEED_DSQ"]}
    assert _lib.SCORES == {s: consts["KS_SCORE_" + s.upper()] for s in ("log2", "pm1", "rank")}
    parts = {n[len("KS_TABLE_PART_"):].lower(): v for n, v in consts.items() if n.startswith("KS_TABLE_PART_")}
    assert {p: i for p, (i, _) in _lib.TABLE_PARTS.items()} == parts


# ----------------------------------------------------------- missing symbols

class _Fn:
    argtypes = restype = "untyped"


def test_typing_skips_a_name_the_library_lacks():
    class StandIn:
        pass
    L = StandIn()
    for name in _lib.EXPORTS:
        if name != "ks_kept_codes_layout":
            setattr(L, name, _Fn())
    _lib._type_library(L, _lib.SIGNATURES)  # does not raise
    for name, (args, res) in _lib.SIGNATURES.items():
        if name != "ks_kept_codes_layout":
            f = getattr(L, name)
            assert f.argtypes is args and f.restype is res, name
    with pytest.raises(AttributeError):  # the call of the missing one still fails at the call
        L.ks_kept_codes_layout(1, 1, 0, 0, None, None)


# ---------------------------------------------------------------- precedence

COUNTS = np.arange(20, dtype=np.uint32).reshape(5, 4) + 1   # 5 x 4
DIST = np.arange(1.0, 7.0)                                  # the 6 entries of n = 4
BAD_COUNTS = COUNTS.astype(np.float64)
NEG_COUNTS = COUNTS.astype(np.int64) - 5
BAD_ROWS = np.zeros((2, 2), dtype=np.int64)
BAD_DIST = np.ones((2, 3))
BAD_GROUP = np.ones((2, 2), dtype=np.int64)

E_COUNTS = "counts must be a [n, ncol] matrix of integer counts"
E_RANGE = "counts must be in the uint32 range"
E_ROWS = "rows must be a 1-d array of integer row indices"
E_ROWS_B = "rows_b must be a 1-d array of integer row indices"
E_DIST = "dist must be a 1-d condensed dissimilarity vector"
E_FIVE2 = "a condensed vector holds n(n-1)/2 entries for some n >= 2; 5 is no such number"
E_FIVE3 = "a condensed vector holds n(n-1)/2 entries for some n >= 3; 5 is no such number"
E_GROUP = "group must hold one integer label for each of the 4 observations"

# (call, the error the parent commit raises first): two bad arguments at once
PRECEDENCE = [
    (lambda: api.region_distances(BAD_COUNTS, rows=BAD_ROWS), E_COUNTS),
    (lambda: api.region_distances(NEG_COUNTS, rows=BAD_ROWS), E_RANGE),
    (lambda: api.region_distances(COUNTS, rows=BAD_ROWS, rows_b=BAD_ROWS), E_ROWS),
    (lambda: api.region_distances(BAD_COUNTS, rows_b=BAD_ROWS), E_COUNTS),
    (lambda: api.region_pca(BAD_COUNTS, rows=BAD_ROWS), E_COUNTS),
    (lambda: api.region_pca(NEG_COUNTS, rows=BAD_ROWS), E_RANGE),
    (lambda: api.region_pca(COUNTS, rows=BAD_ROWS, ncomp=99), E_ROWS),
    (lambda: api.region_kmeans(BAD_COUNTS, [0, 1], rows=BAD_ROWS), E_COUNTS),
    (lambda: api.region_kmeans(COUNTS, np.ones((2, 3)), rows=BAD_ROWS), E_ROWS),
    (lambda: api.region_group_means(BAD_COUNTS, [1, 1, 2, 2, 2], rows=BAD_ROWS), E_COUNTS),
    (lambda: api.region_group_means(COUNTS, BAD_GROUP, rows=BAD_ROWS), E_ROWS),
    (lambda: api.region_kmeans_seed(BAD_COUNTS, 2, rows=BAD_ROWS), E_COUNTS),
    (lambda: api.region_kmeans_seed(COUNTS, "two", rows=BAD_ROWS), E_ROWS),
    (lambda: api.region_knn(BAD_COUNTS, 2, rows=BAD_ROWS), E_COUNTS),
    (lambda: api.region_knn(COUNTS, "two", rows=BAD_ROWS, rows_b=BAD_ROWS), E_ROWS),
    (lambda: api.region_knn(COUNTS, "two", rows_b=BAD_ROWS), E_ROWS_B),
    (lambda: api.region_hclust(BAD_DIST, method="ward"), E_DIST),
    (lambda: api.region_hclust(DIST[:5], method="ward"), E_FIVE2),
    (lambda: api.region_nj(BAD_DIST), E_DIST),
    (lambda: api.region_nj(DIST[:5]), E_FIVE3),
    (lambda: api.region_silhouette(BAD_DIST, BAD_GROUP), E_DIST),
    (lambda: api.region_silhouette(DIST[:5], BAD_GROUP), E_FIVE2),
    (lambda: api.region_silhouette(DIST, BAD_GROUP, ngroups=0), E_GROUP),
]


@pytest.mark.parametrize("case", range(len(PRECEDENCE)))
def test_first_error_of_two_bad_arguments(case, monkeypatch):
    """The first error is the parent commit's, raised before the library is asked for."""
    def no_library():
        raise AssertionError("the library was reached before the arguments were checked")
    monkeypatch.setattr(api, "load", no_library)
    call, text = PRECEDENCE[case]
    with pytest.raises(api.KmerSpansError) as e:
        call()
    assert str(e.value) == text
