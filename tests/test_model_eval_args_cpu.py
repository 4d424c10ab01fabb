"""``_abi.MODEL_EVAL_ARGS``, the one table of the arguments of the blsq_model_eval*_dev entries, against the prototypes of
include/blsq.h; ``_abi.model_eval_args`` in its two modes; and the call by name of tests/_model_eval.py against a
recording library.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from bounded_lsq import _abi

import _model_eval as me
from test_fit_pipeline_cpu import RecordingContext

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = list(_abi.MODEL_EVAL_ARGS)

# header name -> table name: the d of a device pointer goes; dX (dP in the first entry) is X; G is B
ALIAS = dict(dt="t", dy="y", dw="w", df="f", dJ="J", dmask="mask", dPfix="Pfix", dX="X", dP="X", G="B")


def prototypes():
    """name -> [(C type, parameter name), ...] behind ctx, of every blsq_model_eval*_dev of the header."""
    src = open(os.path.join(ROOT, "include", "blsq.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    out = {}
    for name, params in re.findall(r"\bint\s+(blsq_model_eval\w*_dev)\s*\(([^)]*)\)\s*;", src):
        pairs = [re.fullmatch(r"\s*(.*?[\s*])(\w+)\s*", p).groups() for p in params.split(",")]
        assert pairs[0][1] == "ctx"
        out[name] = [(" ".join(t.replace("*", " * ").split()), p) for t, p in pairs[1:]]
    return out


PROTOTYPES = prototypes()


def test_the_table_has_exactly_the_entries_of_the_header():
    assert len(PROTOTYPES) == 8
    assert set(_abi.MODEL_EVAL_ARGS) == set(PROTOTYPES)


@pytest.mark.parametrize("entry", ENTRIES)
def test_names_and_order_are_the_prototype_s(entry):
    names = [ALIAS.get(p, p) for _, p in PROTOTYPES[entry]]
    assert len(set(names)) == len(names), names              # the aliases merge no two parameters of one prototype
    assert list(_abi.MODEL_EVAL_ARGS[entry]) == names


@pytest.mark.parametrize("entry", ENTRIES)
def test_the_type_is_a_function_of_the_name_and_fits_the_prototype(entry):
    """int -> c_int, long -> c_long; a device pointer (d...) -> void*; a host table -> its typed pointer."""
    restype, argtypes = _abi.SIGNATURES[entry]
    names = _abi.MODEL_EVAL_ARGS[entry]
    assert restype is C.c_int and argtypes[0] is _abi.vp and len(argtypes) == 1 + len(names) == 1 + len(PROTOTYPES[entry])
    assert argtypes[1:] == [_abi.MODEL_EVAL_TYPES[k] for k in names]
    for (ctype, param), k in zip(PROTOTYPES[entry], names):
        if ctype in ("int", "long"):
            want = {"int": C.c_int, "long": C.c_long}[ctype]
        elif param.startswith("d") and param in ALIAS:
            assert ctype in ("const double *", "double *", "const int32_t *")
            want = _abi.vp
        else:
            want = {"const int32_t *": _abi.c_int32_p, "const double *": _abi.c_double_p}[ctype]
        assert _abi.MODEL_EVAL_TYPES[k] is want, (entry, param, k)
    assert set(_abi.MODEL_EVAL_TYPES) == set(_abi.MODEL_EVAL_ARGS["blsq_model_eval_tie_dev"])


def full(**over):
    """Every name at its neutral value (n = nf = 4; the data names hold tags), then `over`."""
    v = dict(est=0, sampling=0, nan_policy=0, model=-1, ncomp=0, fam=None, cnt=None, S=0, shared=None, t_sstride=0, B=1,
             reps=1, m=4, n=4, nf=4, pmap=None, tie_ratio=None, tie_offset=None, t="t", t_stride=0, y="y", w="w",
             w_stride=0, X="X", Pfix=None, f="f", J="J", mask="mask")
    v.update(over)
    return v


# (an entry, a name it does not take, a value it cannot place): one of each kind
UNPLACEABLE = [
    ("blsq_model_eval_dev", "est", 1), ("blsq_model_eval_est_dev", "sampling", 1), ("blsq_model_eval_bin_dev", "nan_policy", 1),
    ("blsq_model_eval_comp_dev", "model", 2), ("blsq_model_eval_map_dev", "ncomp", 1), ("blsq_model_eval_map_dev", "fam", "p"),
    ("blsq_model_eval_dev", "cnt", "p"), ("blsq_model_eval_nan_dev", "S", 2), ("blsq_model_eval_nan_dev", "shared", "p"),
    ("blsq_model_eval_bin_dev", "t_sstride", 4), ("blsq_model_eval_dev", "pmap", "p"), ("blsq_model_eval_dev", "nf", 3),
    ("blsq_model_eval_dev", "Pfix", "p"), ("blsq_model_eval_global_dev", "tie_ratio", "p"),
    ("blsq_model_eval_global_dev", "tie_offset", "p"),
]


@pytest.mark.parametrize("entry,name,value", UNPLACEABLE, ids=["%s-%s" % (e[16:-4] or "plain", k) for e, k, _ in UNPLACEABLE])
def test_strict_refuses_what_the_entry_cannot_place_and_lenient_drops_it(entry, name, value):
    assert name not in _abi.MODEL_EVAL_ARGS[entry]
    values = full(**{name: value})
    with pytest.raises(ValueError, match=r"%s takes no `%s`" % (entry, name)):
        _abi.model_eval_args(entry, values)
    want = [values[k] for k in _abi.MODEL_EVAL_ARGS[entry]]
    assert _abi.model_eval_args(entry, values, strict=False) == want
    # at its neutral value, or absent, the name is no obstacle
    assert _abi.model_eval_args(entry, full()) == want
    del values[name]
    assert _abi.model_eval_args(entry, values) == want


@pytest.mark.parametrize("entry", ENTRIES)
def test_values_pass_through_verbatim_and_names_are_checked(entry):
    """Inconsistent values of the entry's own names are handed on as they are (the argument-error tests rely on it); a
    name of no entry and a missing one are TypeErrors in both modes."""
    odd = full(B=0, reps=-1, nf=99, t=None)
    for strict in (True, False):
        got = _abi.model_eval_args(entry, {k: odd[k] for k in _abi.MODEL_EVAL_ARGS[entry]}, strict)
        assert got == [odd[k] for k in _abi.MODEL_EVAL_ARGS[entry]]
        with pytest.raises(TypeError, match="t_strid"):
            _abi.model_eval_args(entry, full(t_strid=0), strict)
        short = full()
        del short["X"]
        with pytest.raises(TypeError, match="needs X"):
            _abi.model_eval_args(entry, short, strict)


@pytest.mark.parametrize("entry", ENTRIES)
def test_call_places_every_name_where_the_prototype_declares_it(entry):
    """``_model_eval.call`` against a recording library: a distinct tag per name arrives at the position of the
    prototype's parameter of that name, behind the context's handle; the names the entry does not take are dropped."""
    tags = {k: 1000 + i for i, k in enumerate(_abi.MODEL_EVAL_TYPES)}
    ctx = RecordingContext()
    assert me.call(ctx, entry, **tags) == 0
    (name, args), = ctx.lib.calls
    assert name == entry and args[0] is ctx.h and len(args) == 1 + len(PROTOTYPES[entry])
    for pos, (_, param) in enumerate(PROTOTYPES[entry], start=1):
        assert args[pos] == tags[ALIAS.get(param, param)], (entry, pos, param)
    if len(PROTOTYPES[entry]) < len(tags):                 # strict: the tags are no neutral values
        with pytest.raises(ValueError):
            me.call(ctx, entry, True, **tags)


def test_call_turns_host_tables_into_typed_pointers():
    """Sequences and arrays given for fam, cnt, shared, pmap and the tie pair arrive as int32 / double pointers to their
    values, readable while the entry runs."""
    names = _abi.MODEL_EVAL_ARGS["blsq_model_eval_tie_dev"]
    sizes = dict(fam=2, cnt=2, pmap=4, shared=2, tie_ratio=4, tie_offset=4)
    seen = {}

    class Lib:
        @staticmethod
        def blsq_model_eval_tie_dev(h, *args):
            got = dict(zip(names, args))
            seen.update({k: (type(got[k]), got[k][:n]) for k, n in sizes.items()}, Pfix=got["Pfix"], t=got["t"])
            return 0

    class Ctx:
        h, lib = object(), Lib()
    values = full(ncomp=2, fam=(0, 4), cnt=[1, 2], pmap=np.array([0, -1, 1, 1]), tie_ratio=[1.0, 0.5, 2.0, 1.0],
                  tie_offset=(0.0, 0.25, 0.0, 0.0), shared=[1, 0])
    assert me.call(Ctx, "blsq_model_eval_tie_dev", True, **values) == 0
    for k in sizes:
        assert seen[k] == (_abi.MODEL_EVAL_TYPES[k], list(values[k]))
    assert seen["Pfix"] is None and seen["t"] == "t"
