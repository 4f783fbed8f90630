"""The C ABI as include/gemnet_hip.h declares it: integer constants, structs as ctypes classes and, per function, the
return type and (name, ctypes type, happens-before kind) of every parameter.  The header is the only list: `_lib` binds
what this module reads, `hbcheck` takes the kinds.  A type the reader does not know raises; nothing defaults."""
import ctypes
import functools
import os
import re
import types

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gemnet_hip.h")
_SCALARS = {"int": ctypes.c_int, "float": ctypes.c_float, "double": ctypes.c_double, "int64_t": ctypes.c_int64}
_TABLES = ("gn_pack_job", "gn_tn_problem", "gn_tn_target")     # rows of device tables: plain data to a launch


def _strip_comments(text):
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    return re.sub(r"//[^\n]*", " ", text)


def _param_kind(typ, name):
    """Type and name of a parameter / field -> 'r' / 'w' (pointer to const / to mutable data), 'ra' / 'wa' (host array of
    pointers to const / mutable data), 'struct:<type>' (pointer to a struct), 'stream', or None (a value)."""
    stars = typ.count("*")
    if stars == 0:
        return None
    if name == "stream":
        return "stream"
    base = typ.replace("*", " ").replace("const", " ").split()
    if stars == 2:
        return "ra" if typ.startswith("const") else "wa"
    if base and base[0].startswith("gn_") and base[0] not in _TABLES:
        return "struct:" + base[0]
    return "r" if re.match(r"const\b", typ) else "w"


def _split(decl):
    """`const float* A` / `gn_chain_op ops[GN_CHAIN_MAX_OPS]` -> (type, name, array length or None)."""
    decl = decl.strip()
    m = re.search(r"([A-Za-z_]\w*)\s*(?:\[(\w+)\])?$", decl)
    return decl[:m.start()].strip(), m.group(1), m.group(2)


def parse(text):
    """Header text -> namespace(consts {name: int}, structs {name: ctypes.Structure class}, kinds {struct: [(field, kind)]},
    funcs {name: (restype, [(param, ctypes type, kind)])})."""
    text = _strip_comments(text)
    consts = {n: int(v, 0) for n, v in re.findall(r"^[ \t]*#define[ \t]+(GN_\w+)[ \t]+(0x[0-9a-fA-F]+|\d+)[ \t]*$", text, flags=re.M)}
    for body in re.findall(r"\benum\s*\{(.*?)\}", text, flags=re.S):
        consts.update((n, int(v, 0)) for n, v in re.findall(r"(GN_\w+)\s*=\s*(\w+)", body))
    structs, kinds = {}, {}

    def declare(decl, where):
        typ, name, dim = _split(decl)
        ct = ctypes.c_void_p if "*" in typ else _SCALARS.get(typ) or structs.get(typ)
        if ct is None:
            raise TypeError(f"include/gemnet_hip.h: unknown type {typ!r} of {name!r} in {where}")
        if dim:
            ct = ct * (consts[dim] if dim in consts else int(dim))
        return name, ct, _param_kind(typ, name)

    for body, sname in re.findall(r"typedef\s+struct\s*\{(.*?)\}\s*(\w+)\s*;", text, flags=re.S):
        fields = []
        for stmt in filter(None, (s.strip() for s in body.split(";"))):
            first, *more = stmt.split(",")                     # `int M, N, K`: the later declarators share the first one's type
            base = _split(first)[0].rstrip("* ")
            fields += [declare(d, sname) for d in [first] + [base + " " + d for d in more]]
        structs[sname] = type(sname, (ctypes.Structure,), {"_fields_": [(n, ct) for n, ct, _ in fields]})
        kinds[sname] = [(n, k) for n, _, k in fields if k is not None]
    funcs = {}
    for ret, name, params in re.findall(r"^[ \t]*(\w[\w \t\*]*?)\s*\b(gn_\w+)\s*\(([^;{()]*)\)\s*;", text, flags=re.M):
        restype = ctypes.c_char_p if ret.split() == ["const", "char*"] else _SCALARS.get(ret)
        if restype is None:
            raise TypeError(f"include/gemnet_hip.h: unknown return type {ret!r} of {name}")
        funcs[name] = (restype, [declare(p, name) for p in (q.strip() for q in params.split(",")) if p and p != "void"])
    return types.SimpleNamespace(consts=consts, structs=structs, kinds=kinds, funcs=funcs)


@functools.lru_cache(maxsize=None)
def read(path=HEADER):
    """The parsed header; read once per process."""
    with open(path) as f:
        return parse(f.read())


def parse_header(path=HEADER):
    """-> (functions {name: [(param, kind)]}, structs {name: [(pointer field, kind)]}): what hbcheck needs of the C ABI."""
    abi = read(path)
    return {name: [(p, k) for p, _, k in params] for name, (_, params) in abi.funcs.items()}, dict(abi.kinds)
