#!/usr/bin/env python3
"""Golden vectors for the Spaceranger readers: writes the two small trees of tests/sparse_counts_ref.py (TREES) into a temporary
directory and records what the REFERENCE's find_feature_matrix_files / read_feature_matrix / read_feature_names return for
them (tests/golden/visium_count_readers.npz).  Build container only (imports the reference checkout, read-only); its imports
that are absent there (anndata, torchvision, tqdm, ...) get empty stand-in modules: the three readers use none of them.

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_counts.py
"""
import importlib
import os
import sys
import tempfile
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.environ.get('GRIDNEXT_REFERENCE', '/root/reference'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.dont_write_bytecode = True


class _Anything(types.ModuleType):
    """A stand-in module: any attribute is a class that can be called, subclassed and imported from."""
    def __getattr__(self, name):
        if name.startswith('__'):
            raise AttributeError(name)
        return type(name, (), {'__init__': lambda self, *a, **k: None})


for name in ('anndata', 'torchvision', 'torchvision.transforms', 'tqdm', 'hexagdly', 'skimage', 'seaborn'):
    try:
        importlib.import_module(name)
    except ImportError:
        sys.modules[name] = _Anything(name)

from gridnext.visium_datasets import read_feature_matrix, read_feature_names      # noqa: E402
from gridnext.utils import find_feature_matrix_files                               # noqa: E402
from sparse_counts_ref import TREES, write_spaceranger_tree                        # noqa: E402

out = {}
with tempfile.TemporaryDirectory() as tmp:
    for k, spec in enumerate(TREES):
        srd = write_spaceranger_tree(tmp, **spec)[0]
        found = find_feature_matrix_files(srd)
        frame = read_feature_matrix(srd)
        names = read_feature_names(srd)
        out['found_%d' % k] = np.array([os.path.relpath(found[key], srd) for key in ('matrix', 'features', 'barcodes')])
        out['matrix_%d' % k] = np.asarray(frame.sparse.to_dense().values, dtype=np.int64)
        out['genes_%d' % k] = np.array(list(frame.index))
        out['barcodes_%d' % k] = np.array(list(frame.columns))
        out['names_index_%d' % k] = np.array(list(names.index))
        out['names_symbol_%d' % k] = np.array(list(names['gene_symbol']))
dest = os.path.join(ROOT, 'tests', 'golden', 'visium_count_readers.npz')
np.savez_compressed(dest, **out)
print('wrote', dest, {k: v.shape for k, v in out.items()})
