"""The layout of the engine (the package ``laplace_gnn_amd.engine``): the surface of the one-file module it replaced, the C
entries it refers to, which methods synchronise the parameter versions, no lazily created state and no function-body imports.
Source checks only (construction needs a GPU).  No GPU."""
import ast
import glob
import inspect
import os
import re

import laplace_gnn_amd as lg
from laplace_gnn_amd import _lib
from laplace_gnn_amd import engine as en
from conftest import ROOT

PACKAGE = os.path.join(ROOT, "laplace-gnn_amd", "engine")
# the one-file module's ``GraphEngine``: ``str(inspect.signature(...))`` of every public method, "property" for a property
SIGNATURES = {'adj_to_edge_index': "(self) -> 'torch.Tensor'",
              'adjgrad_batch': "(self, idx, y, gammas_B, grad_P: 'torch.Tensor', out_bar: 'torch.Tensor', fork_exact: 'bool' = True, "
                               "loss_scale: 'float' = 1.0, cand=None)",
              'adjgrad_batch_dense': "(self, idx, y, gammas_B, out_bar: 'torch.Tensor', grad_dense: 'torch.Tensor', fork_exact: 'bool' = "
                                     "True, loss_scale: 'float' = 1.0)",
              'adjgrad_finish': "(self, out_bar: 'torch.Tensor', gammas_A, a_scale: 'float', grad_P: 'torch.Tensor', cand=None)",
              'adjgrad_finish_dense': "(self, out_bar: 'torch.Tensor', gammas_A, a_scale: 'float', grad_dense: 'torch.Tensor')",
              'batch_cache_clear': '(self)',
              'batch_cache_stats': "(self) -> 'dict'",
              'bind': "(self, X: 'torch.Tensor', weights: 'Sequence[torch.Tensor]', biases: 'Sequence[torch.Tensor]', act: 'str' = "
                      "'relu', likelihood: 'str' = 'classification', res_weights=None, res_biases=None, norm=None, norm_weight=None, "
                      "norm_bias=None, norm_mean=None, norm_var=None, norm_eps: 'float' = 1e-05)",
              'block_gram': "(self, A: 'torch.Tensor', B: 'torch.Tensor | None' = None) -> 'torch.Tensor'",
              'check_async_errors': '(self)',
              'close': '(self)',
              'device_bytes': "(self) -> 'int'",
              'diag_accumulate': "(self, idx, y, diag: 'torch.Tensor', loss: 'torch.Tensor')",
              'diag_adjgrad_batch': "(self, idx, y, gamma: 'torch.Tensor', grad_P: 'torch.Tensor', out_bar: 'torch.Tensor', h1_bar: "
                                    "'torch.Tensor', e_bar: 'torch.Tensor', loss_scale: 'float' = 1.0, cand=None)",
              'diag_adjgrad_batch_dense': "(self, idx, y, gamma: 'torch.Tensor', out_bar: 'torch.Tensor', h1_bar: 'torch.Tensor', e_bar: "
                                          "'torch.Tensor', grad_dense: 'torch.Tensor', loss_scale: 'float' = 1.0)",
              'diag_adjgrad_finish': "(self, out_bar: 'torch.Tensor', h1_bar: 'torch.Tensor', e_bar: 'torch.Tensor', grad_P: "
                                     "'torch.Tensor', cand=None)",
              'diag_adjgrad_finish_dense': "(self, out_bar: 'torch.Tensor', h1_bar: 'torch.Tensor', e_bar: 'torch.Tensor', grad_dense: "
                                           "'torch.Tensor')",
              'ef_accumulate': "(self, idx, y_seed, y_loss=None, resid_scale: 'float' = 1.0, scale: 'float' = 1.0, diag: 'torch.Tensor | "
                               "None' = None, full: 'torch.Tensor | None' = None, grads: 'bool' = False, loss: 'torch.Tensor | None' = "
                               'None)',
              'enable_kernel_timing': "(self, on: 'bool' = True)",
              'export_adj': '(self)',
              'export_propagation': '(self)',
              'feature_token': '(self)',
              'forward': "(self, idx: 'torch.Tensor') -> 'torch.Tensor'",
              'forward_all': "(self) -> 'torch.Tensor'",
              'full_accumulate': "(self, idx, y, H: 'torch.Tensor', loss: 'torch.Tensor')",
              'full_adjgrad_batch': "(self, idx, y, Gamma: 'torch.Tensor', grad_P: 'torch.Tensor', out_bar: 'torch.Tensor', h1_bar: "
                                    "'torch.Tensor', e_bar: 'torch.Tensor', loss_scale: 'float' = 1.0, cand=None)",
              'full_directions': "(self, idx: 'torch.Tensor', Gamma: 'torch.Tensor')",
              'ggn_matmat_': "(self, G: 'torch.Tensor', loss_buf: 'torch.Tensor', idx, y, V: 'torch.Tensor', from_jacobians: 'bool' = "
                             'False)',
              'glm_covariance': "(self, idx_a: 'torch.Tensor', idx_b: 'torch.Tensor | None' = None, *, QA, QB, S, from_jacobians: 'bool' "
                                "= False) -> 'torch.Tensor'",
              'glm_covariance_chunk_pairs': "(self) -> 'int'",
              'glm_variance': "(self, idx: 'torch.Tensor', S0, S1, kappa, QA0=None, QB0=None, QA1=None, QB1sq=None, out_map=None)",
              'glm_variance_ext': "(self, idx: 'torch.Tensor', S0, S1, kappa, QA0=None, QB0=None, QA1=None, QB1sq=None, Sr=None, "
                                  'QAr=None, QBr=None, out_map=None)',
              'gp_jvp': "(self, idx: 'torch.Tensor', v: 'torch.Tensor') -> 'torch.Tensor'",
              'gp_kernel': "(self, idx_a: 'torch.Tensor', idx_b: 'torch.Tensor', independent: 'bool' = False, matched: 'bool' = False, "
                           "from_jacobians: 'bool' = False) -> 'torch.Tensor'",
              'has_extras': 'property',
              'invalidate': '(self)',
              'is_symmetric': 'property',
              'jacobians': "(self, idx: 'torch.Tensor')",
              'jacobians_subset': "(self, idx: 'torch.Tensor', subnet: 'torch.Tensor')",
              'jvp_block': "(self, idx: 'torch.Tensor', V: 'torch.Tensor') -> 'torch.Tensor'",
              'kernel_timing': '(self)',
              'kernel_timing_launches': '(self)',
              'kfac_accumulate': "(self, idx, y, n_train: 'int', views, loss, fork_exact: 'bool' = True, fuse: 'bool' = True, classes: "
                                 "'tuple[int, int] | None' = None, paths: 'bool | None' = None, share: 'tuple[int, int, int] | None' = "
                                 'None)',
              'kfac_accumulate_fisher': "(self, idx, y_seed, y_loss, n_train: 'int', views, loss, resid_scale: 'float' = 1.0, b_scale: "
                                        "'float' = 1.0, fuse: 'bool' = True)",
              'kfac_plan': "(self, fuse: 'bool' = True, paths: 'bool | None' = None) -> 'dict'",
              'last_kfac_top_kernel': 'property',
              'last_kfac_top_on_tiles': 'property',
              'last_kfac_used_paths': 'property',
              'lastlayer_diag_accumulate': "(self, idx, y, diag: 'torch.Tensor', loss: 'torch.Tensor')",
              'lastlayer_features': "(self, idx: 'torch.Tensor')",
              'lastlayer_full_accumulate': "(self, idx, y, H: 'torch.Tensor', loss: 'torch.Tensor')",
              'lastlayer_kron_accumulate': "(self, idx, y, n_train: 'int', A: 'torch.Tensor', B: 'torch.Tensor', Bb: 'torch.Tensor', "
                                           "loss: 'torch.Tensor', fork_exact: 'bool' = True)",
              'lastlayer_pairs_accumulate': "(self, idx, y, S: 'torch.Tensor', Sb: 'torch.Tensor', loss: 'torch.Tensor')",
              'lastlayer_pairs_place': "(self, S: 'torch.Tensor', Sb: 'torch.Tensor', H: 'torch.Tensor')",
              'likelihood': 'property',
              'lora_grad': "(self, grad_dense: 'torch.Tensor', A: 'torch.Tensor', B: 'torch.Tensor', scaling: 'float')",
              'lora_threshold': "(self, base_rowptr: 'torch.Tensor', base_col: 'torch.Tensor', A: 'torch.Tensor', B: 'torch.Tensor', "
                                "scaling: 'float', threshold: 'float', symmetric: 'bool') -> 'int'",
              'n_params': 'property',
              'new_kfac_buffers': '(self)',
              'new_lastlayer_kron_buffers': '(self)',
              'new_lastlayer_pair_buffers': '(self)',
              'nnz': 'property',
              'num_layers': 'property',
              'num_long_rows': 'property',
              'peek_async_errors': '(self)',
              'rebind': '(self)',
              'sampled_forward': "(self, idx: 'torch.Tensor', theta: 'torch.Tensor', softmax: 'bool' = False) -> 'torch.Tensor'",
              'sampled_forward_in_scope': 'property',
              'set_likelihood': "(self, likelihood: 'str')",
              'set_workspace_limit': "(self, nbytes: 'int')",
              'subnet_full_accumulate': "(self, idx, y, subnet: 'torch.Tensor', H: 'torch.Tensor', loss: 'torch.Tensor')",
              'supports_shares': 'True',
              'train_backward': "(self, grad_out: 'torch.Tensor', token: 'int | None' = None)",
              'train_forward': "(self, idx: 'torch.Tensor', masks=None, p: 'float' = 0.0) -> 'torch.Tensor'",
              'update_adjacency': "(self, rows: 'torch.Tensor', cols: 'torch.Tensor', state: 'torch.Tensor')"}
MODULE_NAMES = ["GraphEngine", "BatchTagMap", "kfac_plan", "_IdentityKey", "KINDS", "ACTS", "LIKS", "NORMS"]
NEW_NAMES = {"workspace_limit": "property", "act": "property", "train_token": "property", "timing_enabled": "property",
             "capture_token": "(self)"}
# the ``lgnn_*`` names the one-file module referred to (attribute names and whole string constants)
C_ENTRIES = ['lgnn_adj_to_edge_index', 'lgnn_adjgrad_finish', 'lgnn_adjgrad_finish_dense', 'lgnn_batch_cache_drop',
             'lgnn_batch_cache_stats', 'lgnn_bind_extras', 'lgnn_bind_model', 'lgnn_block_gram', 'lgnn_check_async_errors',
             'lgnn_create', 'lgnn_destroy', 'lgnn_device_bytes', 'lgnn_diag_accumulate', 'lgnn_diag_adjgrad_batch',
             'lgnn_diag_adjgrad_batch_dense', 'lgnn_diag_adjgrad_finish', 'lgnn_diag_adjgrad_finish_dense', 'lgnn_ef_accumulate',
             'lgnn_enable_kernel_timing', 'lgnn_export_adj', 'lgnn_export_propagation', 'lgnn_forward', 'lgnn_forward_all',
             'lgnn_full_accumulate', 'lgnn_full_adjgrad_batch', 'lgnn_full_directions', 'lgnn_ggn_matmat', 'lgnn_glm_covariance',
             'lgnn_glm_covariance_chunk_pairs', 'lgnn_glm_variance', 'lgnn_glm_variance_ext', 'lgnn_glm_variance_mapped', 'lgnn_gp_jvp',
             'lgnn_gp_kernel', 'lgnn_invalidate', 'lgnn_is_symmetric', 'lgnn_jacobians', 'lgnn_jacobians_subset', 'lgnn_jvp_block',
             'lgnn_kernel_timing_launches', 'lgnn_kernel_timing_read', 'lgnn_kfac_accumulate_classes', 'lgnn_kfac_accumulate_fisher',
             'lgnn_kfac_accumulate_share', 'lgnn_kfac_adjgrad_batch', 'lgnn_kfac_adjgrad_batch_dense', 'lgnn_kfac_batch_tag',
             'lgnn_kfac_last_route', 'lgnn_kfac_last_top', 'lgnn_kfac_last_top_kernel', 'lgnn_kfac_plan',
             'lgnn_lastlayer_diag_accumulate', 'lgnn_lastlayer_features', 'lgnn_lastlayer_full_accumulate',
             'lgnn_lastlayer_kron_accumulate', 'lgnn_lastlayer_pairs_accumulate', 'lgnn_lastlayer_pairs_place', 'lgnn_lora_grad',
             'lgnn_lora_threshold', 'lgnn_nnz', 'lgnn_num_long_rows', 'lgnn_peek_async_errors', 'lgnn_sampled_forward',
             'lgnn_set_workspace_limit', 'lgnn_subnet_full_accumulate', 'lgnn_train_backward', 'lgnn_train_forward',
             'lgnn_update_adjacency']
# the public methods of the one-file module whose body called ``_sync_versions`` (``glm_variance*`` through ``_glm_variance``)
SYNCS = ['adjgrad_batch', 'adjgrad_batch_dense', 'adjgrad_finish', 'adjgrad_finish_dense', 'diag_accumulate', 'diag_adjgrad_batch',
         'diag_adjgrad_batch_dense', 'diag_adjgrad_finish', 'diag_adjgrad_finish_dense', 'ef_accumulate', 'forward', 'forward_all',
         'full_accumulate', 'full_adjgrad_batch', 'full_directions', 'ggn_matmat_', 'glm_covariance', 'glm_variance',
         'glm_variance_ext', 'gp_jvp', 'gp_kernel', 'jacobians', 'jacobians_subset', 'jvp_block', 'kfac_accumulate',
         'kfac_accumulate_fisher', 'lastlayer_diag_accumulate', 'lastlayer_features', 'lastlayer_full_accumulate',
         'lastlayer_kron_accumulate', 'lastlayer_pairs_accumulate', 'sampled_forward', 'subnet_full_accumulate', 'train_backward',
         'train_forward']
LAZY = ["_graph_edits", "_rebinds", "_train_token", "_train_keep", "_ws_limit", "_timing_on", "_keep"]
GUARDS = ("close", "__del__")  # they run on a half-built object
FRONT = ["laplace/*.py", "adjgrad.py", "models.py", "gp.py", "curvature.py"]


def _modules():
    files = sorted(glob.glob(os.path.join(PACKAGE, "*.py")))
    assert {"__init__", "_marshal", "core", "curvature", "matfree", "structure", "train"} == {os.path.basename(f)[:-3] for f in files}
    return {os.path.basename(f)[:-3]: ast.parse(open(f).read()) for f in files}


def _functions(tree):
    return [n for n in ast.walk(tree) if isinstance(n, (ast.FunctionDef, ast.AsyncFunctionDef))]


def _describe(obj):
    if isinstance(obj, property):
        return "property"
    return str(inspect.signature(obj)) if callable(obj) else repr(obj)


# ---- surface ---------------------------------------------------------------------------------------------------------------
def test_public_surface_is_the_one_file_modules():
    public = {n: _describe(inspect.getattr_static(en.GraphEngine, n)) for n in dir(en.GraphEngine) if not n.startswith("_")}
    assert {n: public.get(n) for n in SIGNATURES} == SIGNATURES
    assert {n: public.get(n) for n in NEW_NAMES} == NEW_NAMES
    assert [n for n in MODULE_NAMES if not hasattr(en, n)] == []
    assert lg.GraphEngine is en.GraphEngine and lg.engine is en
    assert type(en.GraphEngine) is type  # one plain class over plain mixins: no metaclass, no generated methods


def test_no_module_holds_more_than_about_400_lines():
    lines = {os.path.basename(f): len(open(f).read().splitlines()) for f in glob.glob(os.path.join(PACKAGE, "*.py"))}
    assert max(lines.values()) <= 400, lines  # (a family that outgrows this is two families)


# ---- C entries -------------------------------------------------------------------------------------------------------------
def _c_names(node):
    """(attribute names, whole string constants) under ``node`` that name a C entry."""
    attrs = [n.attr for n in ast.walk(node) if isinstance(n, ast.Attribute) and n.attr.startswith("lgnn_")]
    consts = [n.value for n in ast.walk(node) if isinstance(n, ast.Constant) and isinstance(n.value, str)
              and re.fullmatch(r"lgnn_\w+", n.value)]
    return attrs, consts


def test_c_entries_are_the_one_file_modules_and_each_is_spelled_once_per_call_site():
    names, twice = set(), []
    for mod, tree in _modules().items():
        attrs, consts = _c_names(tree)
        names |= set(attrs) | set(consts)
        for call in (n for n in ast.walk(tree) if isinstance(n, ast.Call)):
            callee = call.func.attr if isinstance(call.func, ast.Attribute) else getattr(call.func, "id", "")
            a, c = _c_names(call)
            if callee in ("_call", "_call_host", "_finish"):  # the name goes in as a string, and nowhere else in the call
                passed_on = isinstance(call.args[0], ast.Name)  # (``_finish`` hands its caller's string on)
                assert not a and (len(c) >= 1 or passed_on), (mod, call.lineno)
            elif callee == "check" and set(a) & set(c):
                twice.append((mod, call.lineno))  # ``_lib.check(self.lib.lgnn_x(...), "lgnn_x")``: the helper's job
    assert sorted(names) == C_ENTRIES
    assert [n for n in C_ENTRIES if n not in _lib.SIGNATURES] == []
    assert twice == []
    # the direct calls that are left: by-reference handle, no context, and the queries that return a value, not a code
    direct = {a for tree in _modules().values() for a in _c_names(tree)[0]}
    assert {n for n in direct if _lib.SIGNATURES[n][0] is _lib._i32} == {"lgnn_create", "lgnn_kfac_plan", "lgnn_is_symmetric",
                                                                        "lgnn_kfac_last_route", "lgnn_kfac_last_top",
                                                                        "lgnn_kfac_last_top_kernel"}


# ---- version sync ----------------------------------------------------------------------------------------------------------
def test_the_methods_that_synchronise_versions_are_the_one_file_modules():
    fns = {f.name: f for tree in _modules().values() for f in _functions(tree)}

    def self_calls(fn):
        return {n.func.attr for n in ast.walk(fn) if isinstance(n, ast.Call) and isinstance(n.func, ast.Attribute)
                and isinstance(n.func.value, ast.Name) and n.func.value.id == "self"}

    syncing = {"_sync_versions"}
    while True:  # the shared openers: private helpers that synchronise, directly or through one another
        more = {name for name, fn in fns.items() if name.startswith("_") and self_calls(fn) & syncing} - syncing
        if not more:
            break
        syncing |= more
    assert {"_batch", "_batch_y", "_batch_pair", "_glm_variance"} <= syncing
    assert sorted(n for n, fn in fns.items() if not n.startswith("_") and self_calls(fn) & syncing) == SYNCS


# ---- no lazy state ---------------------------------------------------------------------------------------------------------
def test_no_lazy_attribute_probe_on_self_and_no_function_body_import():
    probes, imports = [], []
    for mod, tree in _modules().items():
        for fn in _functions(tree):
            for n in ast.walk(fn):
                if (isinstance(n, ast.Call) and getattr(n.func, "id", "") in ("getattr", "hasattr") and len(n.args) >= 2
                        and getattr(n.args[0], "id", "") == "self" and isinstance(n.args[1], ast.Constant)
                        and str(n.args[1].value).startswith("_") and fn.name not in GUARDS):
                    probes.append((mod, fn.name, n.lineno))
                if isinstance(n, (ast.Import, ast.ImportFrom)):
                    imports.append((mod, fn.name, n.lineno))
    assert probes == [] and imports == []


def test_the_front_reads_no_underscore_attribute_of_an_engine():
    found = []
    files = sorted(f for pat in FRONT for f in glob.glob(os.path.join(ROOT, "laplace-gnn_amd", pat)))
    assert len(files) > 10
    for path in files:
        for n in ast.walk(ast.parse(open(path).read())):
            private = None
            if isinstance(n, ast.Attribute) and n.attr.startswith("_") and not n.attr.startswith("__"):
                private, owner = n.attr, n.value
            elif (isinstance(n, ast.Call) and getattr(n.func, "id", "") in ("getattr", "hasattr") and len(n.args) >= 2
                  and isinstance(n.args[1], ast.Constant) and str(n.args[1].value).startswith("_")):
                private, owner = n.args[1].value, n.args[0]
            if private and (getattr(owner, "id", None) in ("eng", "engine") or getattr(owner, "attr", None) == "engine"):
                found.append((os.path.relpath(path, ROOT), n.lineno, private))
    assert found == []


def test_init_declares_the_state_that_used_to_appear_on_first_use():
    bare = en.GraphEngine.__new__(en.GraphEngine)
    bare.close()  # (the guard of a half-built object)
    assert [a for a in LAZY if hasattr(bare, a)] == []
    trees = _modules()
    init = next(f for f in _functions(trees["core"]) if f.name == "__init__")
    assigned = {t.attr for n in ast.walk(init) if isinstance(n, ast.Assign) for tt in n.targets for t in ast.walk(tt)
                if isinstance(t, ast.Attribute) and getattr(t.value, "id", "") == "self"}
    assert [a for a in LAZY if a not in assigned] == ["_keep"]  # ``_keep`` is gone: the borrow rule of ``_call`` replaced it
    everywhere = {n.attr for m in trees if m != "_marshal" for n in ast.walk(trees[m]) if isinstance(n, ast.Attribute)
                  and getattr(n.value, "id", "") == "self" and isinstance(n.ctx, ast.Store)}  # (the mixins and the core)
    assert "_keep" not in everywhere and everywhere <= assigned  # no method creates an attribute ``__init__`` does not
