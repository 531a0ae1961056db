"""Build-container check of the drop-in boundary: when the reference's own ``src.registry`` is
imported FIRST (what its ``main.py`` does, reference main.py:18-20), this package registers into the reference's LIVE
tables, so ``get_model("unet")`` of an unmodified reference process returns the HIP-backed model.

The reference module is stood in for by a ``src/registry.py`` written to a temporary directory: its seven table
constants and names come from the capture of the real module in golden/registry_behaviour.json, and its ``Registry``
keeps the captured behaviour (warning on a duplicate, the KeyError text).  The check runs in a child process so the
adoption happens at a clean import."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = json.load(open(os.path.join(ROOT, "tests", "golden", "registry_behaviour.json")))

# singular helper name of each table (get_model <-> MODELS, ...), as listed in the capture's "helpers"
SINGULAR = {"models": "model", "datasets": "dataset", "dataset_builders": "dataset_builder",
            "evaluation_strategies": "evaluation_strategy", "criteria": "criterion", "providers": "provider",
            "plugins": "plugin"}

STAND_IN = '''
class Registry:
    def __init__(self, name):
        self.name = name
        self._entries = {{}}

    def register(self, name, obj=None):
        def bind(o):
            if name in self._entries:
                print(f"Warning: {{name}} is already registered in {{self.name}}")
            self._entries[name] = o
            return o
        return bind if obj is None else bind(obj)

    def get(self, name):
        if name not in self._entries:
            raise KeyError(f"{{name}} is not registered in {{self.name}}")
        return self._entries[name]

    def has(self, name):
        return name in self._entries

    def list_all(self):
        return list(self._entries)

    def clear(self):
        self._entries.clear()

{tables}
'''

CHILD = r"""
import sys
sys.path.insert(0, {ref!r})
import src.registry as ref_registry          # the stand-in reference module, imported before the package
sys.path.insert(0, {root!r})
import multimodal_tta_amd
from multimodal_tta_amd import registry as mine
for table in ("MODELS", "DATASETS", "DATASET_BUILDERS", "EVALUATION_STRATEGIES", "CRITERIA", "PROVIDERS", "PLUGINS"):
    assert getattr(mine, table) is getattr(ref_registry, table), table
from multimodal_tta_amd.models import UNet
from multimodal_tta_amd.evaluation import SegmentationEvaluationStrategy
assert ref_registry.get_model("unet") is UNet
assert ref_registry.get_model("unet_multimodal_deepfusion") is ref_registry.get_model("unet_multimodal_midfusion")
assert ref_registry.get_evaluation_strategy("seg_eval") is SegmentationEvaluationStrategy
assert "entmin_tta" in ref_registry.PLUGINS.list_all() and "seg_supervised_step" in ref_registry.PLUGINS.list_all()
assert ref_registry.get_plugin("entmin_tta") is mine.get_plugin("entmin_tta")
try:
    ref_registry.get_model("no_such_model")
except KeyError as e:
    assert "no_such_model is not registered in models" in str(e)
else:
    raise AssertionError("unknown name must raise KeyError")
print("ADOPTED")
"""


def write_stand_in(dest: str) -> str:
    lines = []
    for const, name in GOLD["tables"]:
        lines.append(f"{const} = Registry({name!r})")
        lines.append(f"def get_{SINGULAR[name]}(name):\n    return {const}.get(name)")
    pkg = os.path.join(dest, "src")
    os.makedirs(pkg)
    open(os.path.join(pkg, "__init__.py"), "w").close()
    with open(os.path.join(pkg, "registry.py"), "w") as fh:
        fh.write(STAND_IN.format(tables="\n".join(lines)))
    return dest


def test_components_register_into_the_references_live_tables(tmp_path):
    ref = write_stand_in(str(tmp_path))
    out = subprocess.run([sys.executable, "-c", CHILD.format(ref=ref, root=ROOT)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "ADOPTED" in out.stdout, out.stdout + out.stderr
