"""-m "not gpu": the *_params builders of crossscalepatchmatch_amd/capi.py.  Each starts from what the library's cspm_*_default_params
writes (pure host logic: it answers without a device), sets any field with the field's C type, and rejects an unknown key."""
import ctypes as C

import pytest

from crossscalepatchmatch_amd import capi

# builder, its Structure, the library's defaults function, the word its TypeError uses, keyword -> field where they differ
BUILDERS = [
    (capi.fit_params, capi.FitParams, "cspm_fit_default_params", "plane-fit", {}),
    (capi.seg_params, capi.SegParams, "cspm_seg_default_params", "segment-plane", {}),
    (capi.geom_params, capi.GeomParams, "cspm_geom_default_params", "reprojection", {}),
    (capi.mesh_params, capi.MeshParams, "cspm_mesh_default_params", "mesh", {}),
    (capi.synth_params, capi.SynthParams, "cspm_synth_default_params", "view-synthesis", {}),
    (capi.smooth_params, capi.SmoothParams, "cspm_smooth_default_params", "smoothing", {"lam": "lambda_", "lambda": "lambda_"}),
    (capi.rect_params, capi.RectParams, "cspm_rect_default_params", "rectification", {}),
]
IDS = [b[0].__name__ for b in BUILDERS]


def _values(p):
    return [repr(getattr(p, name)) for name, _ in p._fields_]  # repr: a default may be NaN (cspm_rect_params)


@pytest.mark.parametrize("builder,cls,defaults,what,aliases", BUILDERS, ids=IDS)
def test_no_arguments_give_the_library_defaults(builder, cls, defaults, what, aliases):
    want = cls()
    assert getattr(capi.load_library(), defaults)(C.byref(want)) == 0
    got = builder()
    assert type(got) is cls and _values(got) == _values(want)
    assert C.string_at(C.addressof(got), C.sizeof(got)) == C.string_at(C.addressof(want), C.sizeof(want))


@pytest.mark.parametrize("builder,cls,defaults,what,aliases", BUILDERS, ids=IDS)
def test_every_field_can_be_set_with_its_c_type(builder, cls, defaults, what, aliases):
    base = builder()
    for name, ctype in cls._fields_:
        keys = [name] + [k for k, field in aliases.items() if field == name]
        for key in keys:
            for given in (3.0, 3):  # an int field given 3.0 holds 3; a double field given 3 holds 3.0
                p = builder(**{key: given})
                value = getattr(p, name)
                assert value == 3 and type(value) is (float if ctype is C.c_double else int), (key, given)
                for other, _ in cls._fields_:
                    assert other == name or repr(getattr(p, other)) == repr(getattr(base, other)), (key, other)
    if cls is capi.FitParams:
        assert builder(max_diff=2.5).max_diff == 2.5 and builder(radius=2.9).radius == 2  # int(): truncation, as before


@pytest.mark.parametrize("builder,cls,defaults,what,aliases", BUILDERS, ids=IDS)
def test_an_unknown_key_is_a_type_error(builder, cls, defaults, what, aliases):
    with pytest.raises(TypeError) as e:
        builder(**{cls._fields_[0][0]: 1, "no_such_field": 1})
    assert str(e.value) == f"unknown {what} parameter 'no_such_field'"


def test_smooth_params_lambda_spellings():
    assert capi.smooth_params(lam=7).lambda_ == capi.smooth_params(**{"lambda": 7}).lambda_ == capi.smooth_params(lambda_=7).lambda_ == 7.0
    with pytest.raises(TypeError, match="unknown smoothing parameter 'lamda'"):
        capi.smooth_params(lamda=1)
