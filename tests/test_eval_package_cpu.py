"""The shape of the ``evaluation`` package: its public names, that ``__init__`` only re-exports them, and that every
module imports from lower layers only, at module top level.  No GPU, milliseconds."""
import ast
import inspect
import os

import bsed_amd.evaluation as ev

PUBLIC = [
    "BsedError",
    # clips
    "post_process", "binarize_median_gpu", "binarize_median_classwise_gpu", "decode_regions_gpu", "MEDIAN_WINDOW_S_CLASSWISE",
    "classwise_median_windows", "get_predictions",
    # recording
    "window_plan", "stitch_windows", "gather_windows", "decode_long_gpu", "detect_recording",
    # events
    "EventLists", "sweep_events_gpu", "EventReference", "MATCH_MAX_REF", "event_counts_gpu", "event_f1",
    # intersection
    "intersection_counts_gpu", "intersection_f1", "psds_rates", "psds_from_rates", "PsdsScore", "PsdsResult",
    # tagging
    "TAG_MASK_MAX_CLASSES", "TagThresholds", "tag_counts_gpu", "tag_masks_gpu", "tag_f1", "TaggingResult", "validate_weak",
    "get_f_measure_by_class", "pseudo_label_frame", "pseudo_label",
    # validation
    "ValidationResult", "validate", "recording_problem", "score_recording", "compute_metrics",
    "compute_psds_from_operating_points",
]
LAYERS = ["_common", "clips", "recording", "events", "intersection", "tagging", "validation", "__init__"]    # bottom first
MAX_LINES = 400


def test_public_names_and_a_facade_that_defines_nothing():
    assert len(PUBLIC) == 41 and len(set(PUBLIC)) == 41
    assert len(ev.__all__) == len(set(ev.__all__)) and set(ev.__all__) == set(PUBLIC)
    package = ev.__name__
    for name in PUBLIC:
        obj = getattr(ev, name)                         # resolves
        if name == "BsedError":
            assert obj.__module__ == "bsed_amd._lib"
        elif inspect.isfunction(obj) or inspect.isclass(obj):       # defined in a module of the package, not in the package
            assert obj.__module__.startswith(package + "."), (name, obj.__module__)
        else:
            assert name in ("MEDIAN_WINDOW_S_CLASSWISE", "MATCH_MAX_REF", "TAG_MASK_MAX_CLASSES")
    tree = ast.parse(open(ev.__file__).read())
    for node in tree.body:                              # a docstring, imports and __all__: nothing else
        is_all = isinstance(node, ast.Assign) and [getattr(t, "id", None) for t in node.targets] == ["__all__"]
        is_doc = isinstance(node, ast.Expr) and isinstance(node.value, ast.Constant) and isinstance(node.value.value, str)
        assert is_all or is_doc or isinstance(node, ast.ImportFrom), ast.dump(node)[:80]


def _sibling_imports(tree):
    """(module name, node) of every import of a module of the package, at any nesting depth"""
    for node in ast.walk(tree):
        if isinstance(node, ast.ImportFrom):
            module = node.module or ""
            if node.level == 2 and (module == "evaluation" or module.startswith("evaluation.")):
                module, level = module[len("evaluation."):], 1          # the long way round to a sibling
            else:
                level = node.level
            if level == 1:
                for target in ([module.split(".")[0]] if module else [a.name for a in node.names]):
                    yield target, node
            elif level == 0 and module.startswith("bsed_amd.evaluation"):
                yield (module.split(".") + ["__init__"])[2], node
        elif isinstance(node, ast.Import):
            for a in node.names:
                if a.name.startswith("bsed_amd.evaluation"):
                    yield (a.name.split(".") + ["__init__"])[2], node


def test_modules_import_from_lower_layers_only_and_at_top_level():
    folder = os.path.dirname(ev.__file__)
    files = sorted(f[:-3] for f in os.listdir(folder) if f.endswith(".py"))
    assert files == sorted(LAYERS)                      # every module has its place in the order
    for name in files:
        source = open(os.path.join(folder, name + ".py")).read()
        assert source.count("\n") <= MAX_LINES, f"{name}.py has more than {MAX_LINES} lines"
        tree = ast.parse(source)
        found = list(_sibling_imports(tree))
        assert found or name == "_common", f"{name}.py imports nothing from the package"
        for target, node in found:
            assert target in LAYERS, f"{name}.py line {node.lineno}: unknown module {target!r}"
            assert LAYERS.index(target) < LAYERS.index(name), f"{name}.py line {node.lineno} imports {target} from below"
            assert node in tree.body, f"{name}.py line {node.lineno}: an import of {target} inside a function"
