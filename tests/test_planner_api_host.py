"""The public surface of gl_gym_amd.planner, pinned: every public method (with str(inspect.signature(...))), static method and property
of Planner, RuleSearch, PolicySearch, RuleParams and MLPSpec, and a docstring on each.  No device is needed: the classes are only
inspected.  SURFACE was generated from the commit before the CEM stages and the theta searches were folded together (_CemStages,
_ThetaSearch), by the function surface() below; a refactoring of planner.py must leave it as it is."""
import inspect

import pytest

SURFACE = {
    "Planner": {
        "__init__": "(self, env, n_candidates: 'int', horizon: 'int', gamma: 'float' = 1.0, crop: 'str' = 'nominal', n_scenarios: "
                    "'Optional[int]' = None, noise_scale: 'Optional[float]' = None, noise: 'str' = 'step', n_tail: 'Optional[int]' = None, "
                    "scenario_seed: 'int' = 0, weather_sigma=None, weather_phi: 'float' = 0.0)",
        "cem": "(self, n_iter: 'int', n_elite: 'int', init_std: 'float' = 0.5, min_std: 'float' = 0.05, alpha: 'float' = 0.1, beta: 'float' = "
               "0.0, carry: 'int' = 0, seed: 'int' = 0, mean_t=None, std_t=None) -> 'Dict[str, Any]'",
        "elites": "(self, n_elite: 'int')",
        "fork": "(self, parent_t=None)",
        "new_scenarios": "(self)",
        "refit": "(self, mean_t, std_t, alpha: 'float', min_std: 'float')",
        "rollout": "(self, actions_t=None, controls_t=None)",
        "sample": "(self, mean_t, std_t, beta: 'float' = 0.0, seed: 'int' = 0, draw_index: 'int' = 0, carry: 'int' = 0)",
        "select": "(self, temperature: 'Optional[float]' = None, sequence: 'bool' = False) -> 'Dict[str, Any]'",
        "set_layout": "(self, layout: 'str')",
        "shift": "(self, fill_std: 'float')",
    },
    "RuleSearch": {
        "SCENARIO_KEYS": "attr tuple",
        "__init__": "(self, env, n_candidates: 'int', horizon: 'int', tune, base=None, gamma: 'float' = 1.0, **scenario_kwargs)",
        "best_controller": "(self, b: 'int' = 0)",
        "cem": "(self, n_iter: 'int', n_elite: 'int', init_std: 'float' = 0.5, min_std: 'float' = 0.05, alpha: 'float' = 0.1, carry: 'int' = "
               "0, seed: 'int' = 0, mean=None) -> 'Dict[str, Any]'",
        "cma": "(self, n_iter: 'int', n_elite: 'Optional[int]' = None, init_sigma: 'float' = 0.3, min_sigma: 'float' = 1e-06, max_sigma: "
               "'float' = 1.0, seed: 'int' = 0, mean=None, resume: 'bool' = False, **overrides) -> 'Dict[str, Any]'",
        "cma_defaults": "static (N: 'int', K: 'int', E: 'int') -> 'Dict[str, Any]'",
        "cma_state": "property",
        "cma_t_base": "property",
        "cma_update": "(self, n_elite: 'Optional[int]' = None, min_sigma: 'float' = 1e-06, max_sigma: 'float' = 1.0, **overrides)",
        "decode": "(self, theta_t)",
        "elites": "(self, n_elite: 'int')",
        "encode": "(self, controller_or_dict)",
        "es": "(self, n_iter: 'int', lr: 'float', lr_std: 'float' = 0.1, init_std: 'float' = 0.3, min_std: 'float' = 0.02, max_std: 'float' "
              "= 1.0, std_decay: 'float' = 1.0, optimizer: 'str' = 'adam', betas=(0.9, 0.999), eps: 'float' = 1e-08, seed: 'int' = 0, "
              "mean=None, resume: 'bool' = False) -> 'Dict[str, Any]'",
        "es_t_base": "property",
        "es_update": "(self, mean_t, std_t, lr, lr_std=0.0, std_decay=1.0, *, min_std, max_std=1.0, optimizer='adam', betas=(0.9, 0.999), "
                     "eps=1e-08)",
        "new_scenarios": "(self)",
        "refit": "(self, mean_t, std_t, alpha: 'float', min_std: 'float')",
        "rollout": "(self, theta_t, record: 'bool' = False)",
        "sample": "(self, mean_t, std_t, seed: 'int' = 0, draw_index: 'int' = 0, carry: 'int' = 0)",
        "sample_cma": "(self, seed: 'int' = 0, draw_index: 'int' = 0)",
        "sample_mirrored": "(self, mean_t, std_t, seed: 'int' = 0, draw_index: 'int' = 0)",
        "select": "(self) -> 'Dict[str, Any]'",
        "theta_of": "(self, controller_or_dict)",
        "utilities": "(self)",
    },
    "PolicySearch": {
        "SCENARIO_KEYS": "attr tuple",
        "__init__": "(self, env, n_candidates: 'int', horizon: 'int', spec: 'MLPSpec', share: 'str' = 'greenhouse', gamma: 'float' = 1.0, "
                    "**scenario_kwargs)",
        "best_theta": "(self, b: 'int' = 0)",
        "cem": "(self, n_iter: 'int', n_elite: 'int', init_std: 'float' = 0.5, min_std: 'float' = 0.02, alpha: 'float' = 0.1, carry: 'int' "
               "= 0, seed: 'int' = 0, mean=None) -> 'Dict[str, Any]'",
        "elites": "(self, n_elite: 'int')",
        "encode": "(self, module_or_arrays)",
        "es": "(self, n_iter: 'int', lr: 'float', lr_std: 'float' = 0.1, init_std: 'float' = 0.1, min_std: 'float' = 0.01, max_std: "
              "'float' = 1.0, std_decay: 'float' = 1.0, optimizer: 'str' = 'adam', betas=(0.9, 0.999), eps: 'float' = 1e-08, seed: 'int' = "
              "0, mean=None, resume: 'bool' = False) -> 'Dict[str, Any]'",
        "es_t_base": "property",
        "es_update": "(self, mean_t, std_t, lr, lr_std=0.0, std_decay=1.0, *, min_std, max_std=1.0, optimizer='adam', betas=(0.9, 0.999), "
                     "eps=1e-08)",
        "evaluate": "(self, theta_row, record: 'bool' = False)",
        "new_scenarios": "(self)",
        "refit": "(self, mean_t, std_t, alpha: 'float', min_std: 'float')",
        "rollout": "(self, theta_t, record: 'bool' = False)",
        "sample": "(self, mean_t, std_t, seed: 'int' = 0, draw_index: 'int' = 0, carry: 'int' = 0)",
        "sample_mirrored": "(self, mean_t, std_t, seed: 'int' = 0, draw_index: 'int' = 0)",
        "select": "(self) -> 'Dict[str, Any]'",
        "utilities": "(self)",
    },
    "RuleParams": {
        "__init__": "(self, tune, base=None)",
        "decode": "(self, theta)",
        "encode": "(self, controller_or_dict)",
        "inside": "(self, controller_or_dict) -> 'bool'",
        "struct": "(self)",
        "values": "(self, controller_or_dict)",
    },
    "MLPSpec": {
        "__init__": "(self, in_dim: 'int', hidden=(), activation: 'str' = 'tanh', squash: 'str' = 'clip', scale=1.0, obs_norm=None)",
        "decode": "(self, theta)",
        "encode": "(self, module_or_arrays)",
        "flat": "(self, theta)",
        "struct": "(self, mean_ptr=None, inv_std_ptr=None)",
    },
}


def surface(cls):
    """{public name (and __init__): its signature, "static " + signature, "property", or "attr " + type name}, inherited ones included."""
    out = {}
    for name in dir(cls):
        if name.startswith("_") and name != "__init__":
            continue
        raw = inspect.getattr_static(cls, name)
        if isinstance(raw, property):
            out[name] = "property"
        elif isinstance(raw, staticmethod):
            out[name] = "static " + str(inspect.signature(raw.__func__))
        elif inspect.isfunction(raw):
            out[name] = str(inspect.signature(raw))
        else:
            out[name] = "attr " + type(raw).__name__
    return out


@pytest.mark.parametrize("cls_name", sorted(SURFACE))
def test_public_surface_is_pinned(cls_name):
    from gl_gym_amd import planner
    got, want = surface(getattr(planner, cls_name)), SURFACE[cls_name]
    assert sorted(got) == sorted(want), f"{cls_name}: public names added {sorted(set(got) - set(want))}, removed {sorted(set(want) - set(got))}"
    for name in want:
        assert got[name] == want[name], f"{cls_name}.{name}"


@pytest.mark.parametrize("cls_name", sorted(SURFACE))
def test_every_public_method_has_a_docstring(cls_name):
    from gl_gym_amd import planner
    cls = getattr(planner, cls_name)
    for name, kind in SURFACE[cls_name].items():
        if name == "__init__" or kind.startswith("attr "):
            continue                          # the constructor's arguments are described in the class docstring or at TomatoVecEnv
        raw = inspect.getattr_static(cls, name)
        doc = (raw.fget if isinstance(raw, property) else getattr(cls, name)).__doc__
        assert doc and doc.strip(), f"{cls_name}.{name} has no docstring"


def test_scenario_keys():
    from gl_gym_amd.planner import PolicySearch, RuleSearch
    keys = ("n_scenarios", "n_tail", "noise", "noise_scale", "scenario_seed", "weather_sigma", "weather_phi")
    assert RuleSearch.SCENARIO_KEYS == keys and PolicySearch.SCENARIO_KEYS == keys
