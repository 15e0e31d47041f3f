"""ngsld_analyze in the C-ABI without a GPU: the symbol is exported, the binding's structs have the layout the header declares
(sizes and field offsets, from the header's own text), and the six kind constants are the header's, distinct and non-zero."""
import ctypes as C
import os
import re

from ngsld_amd import capi

HEADER = os.path.join(capi.REPO_DIR, "include", "ngsld.h")

# the C types the two structs use
CTYPES = {"uint32_t": C.c_uint32, "uint64_t": C.c_uint64, "double": C.c_double}


def _header():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def _struct_from_header(name):
    """A ctypes.Structure with the fields of `typedef struct <name> { ... } <name>;` as a C compiler lays them out."""
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), _header(), flags=re.S).group(1)
    fields = []
    for decl in (d.strip() for d in body.split(";")):
        if not decl:
            continue
        if "*" in decl:  # a pointer of any kind: its name is the last identifier
            fields.append((re.findall(r"\w+", decl)[-1], C.c_void_p))
            continue
        ctype, names = decl.split(None, 1)
        fields += [(n.strip(), CTYPES[ctype]) for n in names.split(",")]
    return type(name, (C.Structure,), {"_fields_": fields})


def _layout(struct):
    return [(n, getattr(struct, n).offset, getattr(struct, n).size) for n, _ in struct._fields_]


def test_ngsld_analyze_is_exported_and_bound():
    assert "ngsld_analyze" in capi.SYMBOLS
    L = capi.lib()
    assert hasattr(L, "ngsld_analyze")
    assert L.ngsld_analyze.argtypes[1] == C.POINTER(capi.Analysis) and L.ngsld_analyze.argtypes[3] == C.POINTER(capi.AnalyzeStats)


def test_structs_have_the_headers_layout():
    for name, bound in (("ngsld_analysis", capi.Analysis), ("ngsld_analyze_stats", capi.AnalyzeStats)):
        want = _struct_from_header(name)
        assert C.sizeof(bound) == C.sizeof(want), name
        assert _layout(bound) == _layout(want), name
    assert C.sizeof(capi.Analysis) == 40 and C.sizeof(capi.AnalyzeStats) == 56


def test_kind_constants_are_the_headers_distinct_and_non_zero():
    m = re.search(r"enum \{ (NGSLD_AN_PRUNE = 1[^}]*)\}", _header())
    names = [x.strip() for x in m.group(1).split(",")]
    assert names[0] == "NGSLD_AN_PRUNE = 1"
    names[0] = "NGSLD_AN_PRUNE"
    header = {n[len("NGSLD_"):]: 1 + k for k, n in enumerate(names)}  # (an enum counts on from its first value)
    bound = {n: getattr(capi, n) for n in ("AN_PRUNE", "AN_DECAY", "AN_SITE_LD", "AN_CLUSTERS", "AN_GRID", "AN_SCAN")}
    assert bound == header
    assert len(set(bound.values())) == 6 and all(v != 0 for v in bound.values())
    # Engine.analyze lists them in the order of its signature
    assert list(capi.ANALYSES.values()) == sorted(capi.ANALYSES.values()) and set(capi.ANALYSES.values()) == set(bound.values())
    import inspect
    assert list(inspect.signature(capi.Engine.analyze).parameters)[1:] == list(capi.ANALYSES)
