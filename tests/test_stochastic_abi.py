"""CPU: the two entry points of the stochastic samplers are additions to the C ABI -- declared in
include/elastic_hip.h and in ``_hip.SIGNATURES`` with matching arity, exported by the built library -- and the ABI number stays 13."""
from elasticdiffusion_official_amd import _hip
from tests.test_abi import header_functions

NEW = {"ed_cfg_ddim_step_sde": "ed_cfg_ddim_step_ms", "ed_phase_epilogue_sde": "ed_phase_epilogue_ms"}


def test_sde_entry_points_are_declared_with_matching_arity():
    declared = dict(header_functions())
    for name, base in NEW.items():
        assert name in declared and name in _hip.SIGNATURES
        n_args = len([a for a in declared[name].split(",") if a.strip()])
        assert n_args == len(_hip.SIGNATURES[name])
        # the *_ms signature plus (int form, float c_n, const float* noise) before the stream
        assert _hip.SIGNATURES[name] == _hip.SIGNATURES[base][:-1] + [_hip._i, _hip._f, _hip._vp] + _hip.SIGNATURES[base][-1:]
        args = [a.strip() for a in declared[name].split(",")]
        assert [a.split()[-1].lstrip("*") for a in args[-4:]] == ["form", "c_n", "noise", "stream"]
        assert [a.split()[-1].lstrip("*") for a in args[:-4]] == [a.strip().split()[-1].lstrip("*") for a in declared[base].split(",")][:-1]


def test_abi_version_is_still_13_and_the_library_exports_them():
    assert _hip.ABI_VERSION == 13
    _hip.build_library()
    L = _hip.lib()
    assert L.ed_version() == 13
    for name in NEW:
        assert hasattr(L, name)
