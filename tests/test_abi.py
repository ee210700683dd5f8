"""The C-ABI library loads without a GPU and exports every symbol include/showtell_hip.h declares, and the hand-written
ctypes mirror in showtell_amd/_lib.py (structs, signatures) agrees with that header.

Each check is a function over plain data (the header text, a _SIGS-like dict, a list of struct classes) that returns the
list of disagreements it found, so the same file feeds it deliberately broken copies and asserts that they are flagged."""
import ctypes
import glob
import os
import re
import subprocess
import tempfile

from tests._util import ROOT

INCLUDE = os.path.join(ROOT, "include")


def _header_text():
    txt = open(os.path.join(INCLUDE, "showtell_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return re.sub(r"#ifdef ST_EXPERIMENTAL.*?#endif", "", txt, flags=re.S)   # `make EXPERIMENTAL=1` entry points are not in the product build


def _header_symbols():
    return sorted(set(re.findall(r"\b(st_[a-z0-9_]+)\s*\(", _header_text())))


# ---- struct layout -----------------------------------------------------------------------------------------------------

def _mirrored_structs():
    from showtell_amd import _lib
    return [(_lib.ConvDesc, "st_conv_desc"), (_lib.Conv3x3ImgDesc, "st_conv3x3_img_desc"), (_lib.Conv1x1WregDesc, "st_conv1x1_wreg_desc"),
            (_lib.Conv1x1KfuseDesc, "st_conv1x1_kfuse_desc"), (_lib.StemConvPoolDesc, "st_stem_conv_pool_desc"),
            (_lib.ConvB2bDesc, "st_conv_b2b_desc"), (_lib.ConvC3c1Desc, "st_conv_c3c1_desc"), (_lib.BnActDesc, "st_bn_act_desc"),
            (_lib.RnnParams, "st_rnn_params"), (_lib.RnnGrads, "st_rnn_grads"), (_lib.AttnParams, "st_attn_params"),
            (_lib.AttnGrads, "st_attn_grads"), (_lib.PackedSeq, "st_packed_seq"), (_lib.ImageBatchDesc, "st_image_batch_desc"),
            (_lib.LossTerms, "st_loss_terms"), (_lib.DropoutDesc, "st_dropout"), (_lib.BeamOpts, "st_beam_opts")]


def layout_errors(structs):
    """structs: [(ctypes.Structure class, C type name)].  A gcc program prints sizeof of each C type and offsetof / sizeof of
    every field BY THE CTYPES FIELD NAME: a field the header does not have fails to compile, a moved or resized one differs."""
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "showtell_hip.h"', 'int main(void) {']
    want = []
    for cls, cname in structs:
        lines.append(f'  printf("%zu\\n", sizeof({cname}));')
        want.append((f"sizeof({cname})", ctypes.sizeof(cls)))
        for field in cls._fields_:
            f = field[0]
            lines.append(f'  printf("%zu %zu\\n", offsetof({cname}, {f}), sizeof((({cname}*)0)->{f}));')
            want.append((f"{cname}.{f}", (getattr(cls, f).offset, getattr(cls, f).size)))
    lines += ['  return 0;', '}']
    with tempfile.TemporaryDirectory() as td:
        src, exe = os.path.join(td, "layout.c"), os.path.join(td, "layout")
        with open(src, "w") as fh:
            fh.write("\n".join(lines) + "\n")
        cc = subprocess.run(["gcc", "-I", INCLUDE, src, "-o", exe], capture_output=True, text=True)
        if cc.returncode != 0:
            return ["does not compile against the header: " + cc.stderr.strip()]
        out = subprocess.check_output([exe], text=True).splitlines()
    errs = []
    for (what, py), line in zip(want, out):
        c = tuple(map(int, line.split()))
        c = c[0] if len(c) == 1 else c
        if c != py:
            errs.append(f"{what}: header {c}, ctypes {py}")
    return errs


# ---- prototypes --------------------------------------------------------------------------------------------------------

_C_SCALARS = ("int", "long", "size_t", "float", "double", "void")


def _c_class(decl, is_param):
    """'const float* x' -> 'pointer', 'size_t workspace_bytes' -> 'size_t', 'int' -> 'int' (the parameter name is optional)."""
    if "*" in decl:
        return "pointer"
    words = [w for w in decl.split() if w != "const"]
    if is_param and len(words) > 1:
        words = words[:-1]
    t = " ".join(words)
    assert t in _C_SCALARS, f"test_abi cannot classify the C type {decl!r}"
    return t


def header_prototypes(text):
    """{name: (return class, [argument classes])} of every `<type> st_name(<params>);` in the (comment-free) header text."""
    protos = {}
    for ret, name, params in re.findall(r"([A-Za-z_][\w \t\*]*?)\b(st_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", text):
        params = [" ".join(p.split()) for p in params.split(",")]
        args = [] if params == ["void"] else [_c_class(p, True) for p in params]
        protos[name] = (_c_class(" ".join(ret.split()), False), args)
    return protos


def _ctypes_class(t):
    """By size and kind, not identity: on Linux c_long is c_int64 and c_size_t is c_ulong."""
    if t is None:
        return "void"
    if issubclass(t, (ctypes._Pointer, ctypes.c_void_p, ctypes.c_char_p)):
        return "pointer"
    code, size = t._type_, ctypes.sizeof(t)
    kind = {"f": "float", "d": "double"}.get(code) or ("signed" if code in "bhilq" else "unsigned" if code in "BHILQ" else code)
    return {("float", 4): "float", ("double", 8): "double", ("signed", ctypes.sizeof(ctypes.c_int)): "int",
            ("signed", ctypes.sizeof(ctypes.c_long)): "long", ("unsigned", ctypes.sizeof(ctypes.c_size_t)): "size_t"}[(kind, size)]


def prototype_errors(protos, sigs):
    """Every prototype that has an entry in `sigs` ({name: ([argtypes], restype)}) must agree with it in arity and in the class
    of each argument and of the return value."""
    errs = []
    for name, (ret, args) in sorted(protos.items()):
        if name not in sigs:
            continue
        pargs, pret = sigs[name]
        pargs, pret = [_ctypes_class(a) for a in pargs], _ctypes_class(pret)
        if len(pargs) != len(args):
            errs.append(f"{name}: header takes {len(args)} arguments, _SIGS {len(pargs)}")
        elif pargs != args:
            errs.append(f"{name}: " + ", ".join(f"argument {i} is {c} in the header, {p} in _SIGS"
                                                for i, (c, p) in enumerate(zip(args, pargs)) if c != p))
        if pret != ret:
            errs.append(f"{name}: returns {ret} in the header, {pret} in _SIGS")
    return errs


def symbol_set_errors(header_symbols, sigs, experimental):
    """Header symbols == keys of `sigs` minus the experimental ones (st_last_error, bound on its own, is part of `sigs` here)."""
    bound = set(sigs) - set(experimental)
    return ([f"{s}: declared in the header, no entry in _SIGS" for s in sorted(set(header_symbols) - bound)]
            + [f"{s}: entry in _SIGS, not declared in the header" for s in sorted(bound - set(header_symbols))])


def unbound_call_sites(texts, sigs):
    """texts: {path: python source}.  Every `.st_<name>(` must name an entry of `sigs`."""
    return [f"{path}: calls {name}, which has no entry in _SIGS" for path, txt in sorted(texts.items())
            for name in sorted(set(re.findall(r"\.(st_[a-z0-9_]+)\s*\(", txt)) - set(sigs))]


def _all_sigs():
    from showtell_amd import _lib
    return {**_lib._SIGS, "st_last_error": ([], ctypes.c_char_p)}


def _python_sources():
    paths = [os.path.join(ROOT, "bench.py"), os.path.join(ROOT, "__graft_entry__.py")]
    for d in ("show-tell_amd", "tests", "tools"):
        paths += glob.glob(os.path.join(ROOT, d, "**", "*.py"), recursive=True)
    return {os.path.relpath(p, ROOT): open(p).read() for p in paths}


# ---- the tests ---------------------------------------------------------------------------------------------------------

def test_library_loads_and_exports_every_declared_symbol():
    from showtell_amd import _lib
    L = _lib.lib()                      # raises ShowTellHipError when the .so is missing: no fallback
    assert L.st_version() >= 1
    syms = _header_symbols()
    assert len(syms) >= 25
    raw = ctypes.CDLL(_lib.LIB_PATH)    # lib() hands out bound entry points only; what the file exports is asked of the file
    for s in syms:
        assert hasattr(raw, s), f"{s} declared in showtell_hip.h but not exported"
        assert hasattr(L, s), f"{s} declared in showtell_hip.h but not bound"
    # every bound signature corresponds to a declared symbol
    assert set(_lib.declared_symbols()) <= set(syms), set(_lib.declared_symbols()) - set(syms)


def test_lib_hands_out_bound_entry_points_only():
    import pytest
    from showtell_amd import _lib
    L = _lib.lib()
    assert set(vars(L)) == {s for s in _all_sigs() if s not in _lib._EXPERIMENTAL or hasattr(ctypes.CDLL(_lib.LIB_PATH), s)}
    assert L.st_conv_c3c1.argtypes == _lib._SIGS["st_conv_c3c1"][0]
    with pytest.raises(AttributeError, match="no entry in _lib._SIGS"):
        L.hipMalloc                     # exported by a dependency, reachable through a bare CDLL, described nowhere
    assert not _lib.has_symbol("st_no_such_entry_point")


def test_struct_sizes_match_the_header():
    """ctypes mirrors of the C structs must have the C compiler's layout (checked with gcc)."""
    from showtell_amd import _lib
    src = ('#include <stdio.h>\n#include "showtell_hip.h"\nint main(){printf("%zu %zu %zu %zu %zu\\n", sizeof(st_conv_desc), '
           'sizeof(st_bn_act_desc), sizeof(st_rnn_params), sizeof(st_rnn_grads), sizeof(st_packed_seq));return 0;}\n')
    with tempfile.TemporaryDirectory() as td:
        c = os.path.join(td, "s.c")
        open(c, "w").write(src)
        exe = os.path.join(td, "s")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        sizes = list(map(int, subprocess.check_output([exe]).split()))
    assert sizes == [ctypes.sizeof(_lib.ConvDesc), ctypes.sizeof(_lib.BnActDesc), ctypes.sizeof(_lib.RnnParams),
                     ctypes.sizeof(_lib.RnnGrads), ctypes.sizeof(_lib.PackedSeq)]


def test_every_mirrored_struct_has_the_headers_layout():
    structs = _mirrored_structs()
    assert len(structs) == 17 and sum(len(c._fields_) for c, _ in structs) == 280
    from showtell_amd import _lib
    mirrored = {c for c, _ in structs}
    assert {v for v in vars(_lib).values() if isinstance(v, type) and issubclass(v, ctypes.Structure) and v is not ctypes.Structure} == mirrored
    assert layout_errors(structs) == []


def test_every_prototype_matches_its_signature():
    protos = header_prototypes(_header_text())
    assert sorted(protos) == _header_symbols()      # the prototype parser saw every declared entry point
    assert len(protos) >= 92                        # 93 with the ST_EXPERIMENTAL one
    assert prototype_errors(protos, _all_sigs()) == []


def test_header_and_signatures_name_the_same_symbols():
    from showtell_amd import _lib
    assert symbol_set_errors(_header_symbols(), _all_sigs(), _lib._EXPERIMENTAL) == []
    assert sorted(set(_all_sigs()) - set(_lib._EXPERIMENTAL)) == _lib.declared_symbols()


def test_every_call_site_names_a_bound_entry_point():
    texts = _python_sources()
    assert len(texts) > 100 and "show-tell_amd/ops.py" in texts and "tools/time_bptt.py" in texts and "bench.py" in texts
    assert unbound_call_sites(texts, _all_sigs()) == []


def test_seeded_faults_are_caught():
    """The checks above, fed a mirror with one deliberate mistake each."""
    from showtell_amd import _lib
    protos, sigs = header_prototypes(_header_text()), _all_sigs()
    args, res = sigs["st_rnn_forward"]
    # an argument dropped from one signature
    errs = prototype_errors(protos, {**sigs, "st_rnn_forward": (args[:-1], res)})
    assert errs == ["st_rnn_forward: header takes 13 arguments, _SIGS 12"]
    # a c_int replaced by a c_float
    i = args.index(ctypes.c_int)
    errs = prototype_errors(protos, {**sigs, "st_rnn_forward": (args[:i] + [ctypes.c_float] + args[i + 1:], res)})
    assert errs == [f"st_rnn_forward: argument {i} is int in the header, float in _SIGS"]
    # ... and a c_size_t return by a c_int one (what ctypes assumes for a function nobody described)
    errs = prototype_errors(protos, {**sigs, "st_rnn_workspace_bytes": (sigs["st_rnn_workspace_bytes"][0], ctypes.c_int)})
    assert errs == ["st_rnn_workspace_bytes: returns size_t in the header, int in _SIGS"]
    # two fields swapped in a struct copy (same types, so every size still agrees)
    fields = list(_lib.Conv3x3ImgDesc._fields_)
    a, b = [n for n, _ in fields].index("scale"), [n for n, _ in fields].index("shift")
    fields[a], fields[b] = fields[b], fields[a]
    swapped = type("Conv3x3ImgDescSwapped", (ctypes.Structure,), {"_fields_": fields})
    errs = layout_errors([(swapped, "st_conv3x3_img_desc")])
    assert len(errs) == 2 and errs[0].startswith("st_conv3x3_img_desc.shift:") and errs[1].startswith("st_conv3x3_img_desc.scale:")
    # a field the header does not have
    renamed = type("PackedSeqRenamed", (ctypes.Structure,), {"_fields_": [(n if n != "ntok" else "n_tok", t) for n, t in _lib.PackedSeq._fields_]})
    errs = layout_errors([(renamed, "st_packed_seq")])
    assert len(errs) == 1 and "does not compile" in errs[0] and "n_tok" in errs[0]
    # an entry deleted from the dict: the header has one symbol more, and its call sites are unbound
    fewer = {k: v for k, v in sigs.items() if k != "st_conv_c3c1"}
    assert symbol_set_errors(_header_symbols(), fewer, _lib._EXPERIMENTAL) == ["st_conv_c3c1: declared in the header, no entry in _SIGS"]
    assert unbound_call_sites({"ops.py": _python_sources()["show-tell_amd/ops.py"]}, fewer) == ["ops.py: calls st_conv_c3c1, which has no entry in _SIGS"]
    # an entry the header does not declare
    assert symbol_set_errors(_header_symbols(), {**sigs, "st_made_up": ([], ctypes.c_int)}, _lib._EXPERIMENTAL) == \
        ["st_made_up: entry in _SIGS, not declared in the header"]


def test_host_side_errors_without_gpu():
    import pytest
    import torch
    from showtell_amd import ShowTellHipError, ops
    with pytest.raises(ShowTellHipError):
        ops.cast(torch.zeros(4), torch.bfloat16)          # CPU tensor -> loud failure, never a fallback
    from showtell_amd.cnn import ResNet
    with pytest.raises(ValueError):
        ResNet(99)
