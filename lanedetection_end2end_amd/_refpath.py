"""Optional: let the mirrored ``Networks`` packages fall through to the reference tree for the
host-side plumbing modules this project does not replace (``Networks.utils``: argparse flags,
optimisers, logging -- SURVEY.md section 2, row 10).  Set LANEFIT_REFERENCE_ROOT to the directory
holding ``Birds_Eye_View_Loss/`` and ``Backprojection_Loss/``; see INTEGRATION.md."""
import os


def extend(pkg_path, tree):
    root = os.environ.get("LANEFIT_REFERENCE_ROOT")
    if root:
        cand = os.path.join(root, tree, "Networks")
        if os.path.isdir(cand) and cand not in pkg_path:
            pkg_path.append(cand)


def load_reference_module(tree, relpath, private_name):
    """The reference's ``tree/relpath`` executed as a module called ``private_name`` (kept out of the name the mirror's own module
    of that path holds in ``sys.modules``), or None when LANEFIT_REFERENCE_ROOT is unset or has no such file.  A mirror module that
    replaces part of a reference module re-exports the rest from this."""
    import importlib.util
    import sys
    root = os.environ.get("LANEFIT_REFERENCE_ROOT")
    if not root:
        return None
    path = os.path.join(root, tree, relpath)
    if not os.path.isfile(path):
        return None
    if private_name in sys.modules:
        return sys.modules[private_name]
    spec = importlib.util.spec_from_file_location(private_name, path)
    module = importlib.util.module_from_spec(spec)
    sys.modules[private_name] = module
    try:
        spec.loader.exec_module(module)
    except BaseException:
        del sys.modules[private_name]
        raise
    return module
