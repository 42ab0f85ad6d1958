"""registry.install_into_reference(): the drop-in really swaps this package's classes into the REFERENCE's registry,
so that the reference's own ``create_model`` (equihgnn/utils/create.py:5-10) -- the call LitModel makes at
main.py:28-34 -- hands back the MI355X classes under the same ``--method`` names.

With the reference checkout at hand, it is imported with the golden generator's recipe (tests/golden/make_golden.py::
import_reference: stand-ins for the absent third-party packages), in a child process so that those stand-ins never enter the
test session's ``sys.modules``.  Without it, the child stands in the reference's registry interface (``registry.mapping
["model_name_mapping"]``, ``get_model_class``, ``create_model`` raising ValueError for unknown names) and holds the swapped
classes to the stock classes' state_dict layouts stored in tests/golden/reference_state_dicts.json (written from the reference
by ``make_golden.py --state-dict-layouts``; with the checkout, the child checks that file against the stock classes)."""
import os
import subprocess
import sys
import textwrap


from common import GOLDEN_DIR

REF = "/root/reference"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = textwrap.dedent('''
    import importlib, json, os, sys, types
    ROOT, GOLD, REF = sys.argv[1:4]
    sys.path[:0] = [ROOT, GOLD]
    import make_golden as mg
    layouts = json.load(open(os.path.join(GOLD, "reference_state_dicts.json")))
    names = mg.INSTALL_METHODS
    if os.path.isdir(os.path.join(REF, "equihgnn")):
        ref_registry = mg.import_reference(("equihnn_egnn", "mhnn"))
        # the reference's create_model, loaded as equihgnn.utils.create without equihgnn/utils/__init__.py (whose
        # data_split import pulls in the dataset stack)
        pkg = types.ModuleType("equihgnn.utils")
        pkg.__path__ = [os.path.join(REF, "equihgnn", "utils")]
        sys.modules["equihgnn.utils"] = pkg
        create = importlib.import_module("equihgnn.utils.create")
        assert os.path.realpath(create.__file__).startswith(os.path.realpath(REF))
        stock = {n: create.create_model(n) for n in names}
        # the stored layouts are the stock classes' own
        assert {n: mg.state_dict_layout(stock[n], n) for n in names} == layouts
    else:
        # stand-in of the reference's registry interface, holding placeholders for its stock classes
        class Registry:
            mapping = {"model_name_mapping": {}}

            @classmethod
            def get_model_class(cls, name):
                return cls.mapping["model_name_mapping"].get(name, None)
        ref_registry = Registry()
        for n in names:
            ref_registry.mapping["model_name_mapping"][n] = type(n, (), {"__module__": "equihgnn.models." + n})
        mods = {m: types.ModuleType(m) for m in ("equihgnn", "equihgnn.common", "equihgnn.common.registry",
                                                 "equihgnn.utils", "equihgnn.utils.create")}
        mods["equihgnn.common.registry"].registry = ref_registry

        def create_model(model_name):
            model_cls = ref_registry.get_model_class(name=model_name)
            if model_cls is None:
                raise ValueError(f"Model with name {model_name} not found.")
            return model_cls
        mods["equihgnn.utils.create"].create_model = create_model
        sys.modules.update(mods)
        create = mods["equihgnn.utils.create"]
        stock = {n: create.create_model(n) for n in names}
    assert all(c.__module__.startswith("equihgnn.models") for c in stock.values())

    from equihgnn_amd import models as M
    from equihgnn_amd.registry import default_args, install_into_reference, registry as mine

    kept = install_into_reference(override=False)          # names the reference already has stay the reference's
    assert not (set(kept) & set(stock)) and create.create_model("egnn_equihnns") is stock["egnn_equihnns"]
    for n in kept:                                          # (names its registry did not hold -- their model files were
        assert create.create_model(n) is M.MODELS[n]        #  not imported here -- are added)

    done = install_into_reference()
    assert sorted(done) == sorted(M.MODELS) == sorted(mine.mapping["model_name_mapping"])
    for n in done:
        assert create.create_model(n) is M.MODELS[n], n
        assert ref_registry.get_model_class(n) is M.MODELS[n], n
    try:
        create.create_model("no_such_method")
    except ValueError as e:
        assert "not found" in str(e)
    else:
        raise AssertionError("unknown names must still raise")

    # main.py:28-34: model_cls = create_model(hparams.method); model_cls(1, hparams) -- same state_dict as the stock class
    # (load_state_dict matches by name: the registration order is free; the layouts are {key: [shape, dtype]})
    for n in stock:
        swapped = create.create_model(n)
        assert swapped.__name__ != "GNN_2D"
        assert mg.state_dict_layout(swapped, n) == layouts[n], n
    print("INSTALL-OK", len(done))
''')


def test_install_into_reference_swaps_the_registry_entries():
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT, GOLDEN_DIR, REF], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "INSTALL-OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
