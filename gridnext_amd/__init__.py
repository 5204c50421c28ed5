"""gridnext_amd - MI355X-native implementation of GridNext's f∘g training hot path.

Public surface mirrors the reference package for that path:
    from gridnext_amd.densenet import DenseNet
    from gridnext_amd.gridnet_models import GridNet, GridNetHex, GridNetHexOddr, GridNetHexMM
    from gridnext_amd.training import train_spotwise, train_gridwise
    from gridnext_amd.multimodal_datasets import MMStackDataset, MultiModalDataset, MultiModalGridDataset
    import gridnext_amd.hexconv as hexagdly          # Conv2d(kernel_size=1, stride=1)
    from gridnext_amd import optim                   # optim.Adam / optim.AdamW: the step as one HIP launch per group
    from gridnext_amd import transforms              # Compose / Resize / CenterCrop / ToTensor / Normalize (for torchvision's)
    from gridnext_amd.imgprocess import grid_from_wsi_visium, save_visium_patches    # whole-slide image -> patch grid
    from gridnext_amd import metrics                 # confusion matrix, ROC / PR curves and AUCs, misclassification map
    from gridnext_amd.visium_datasets import create_visium_counts, SpotCounts, SparseCountDataset, SparseCountGridDataset
    from gridnext_amd.sparse_linear import SparseCountLinear, SparseCountMLP    # the first Linear layer over sparse rows
    from gridnext_amd.count_pca import CountPCA      # what SpotCounts.fit_pca returns: a PCA fitted on the sparse counts
    from gridnext_amd.hvg import HighlyVariableGenes # what SpotCounts.highly_variable_genes returns: Seurat-v3 genes from raw counts
    from gridnext_amd.spatial import SpatialAutocorr # what SpotCounts.spatial_autocorr returns: Moran's I and Geary's C per gene
    from gridnext_amd.expression import SparseMSELoss, ExpressionNet      # expression from patches: sigmoid + MSE on sparse rows (host), the model
    from gridnext_amd.expression import ExpressionMetrics, evaluate_expression    # per-gene Pearson / R^2 / MSE, host or resident counts
    from gridnext_amd.multimodal_datasets import SlideCountDataset        # slide patches paired with sparse count rows
    from gridnext_amd.training import train_expression
All arithmetic runs in hand-written gfx950 kernels behind the C ABI of include/gridnext_hip.h
(libgridnext_hip.so, built in-tree by `__graft_entry__.build()`); there is no CPU fallback.
"""
__version__ = "0.1.0"

from .densenet import DenseNet                                                     # noqa: F401
from .gridnet_models import GridNet, GridNetHex, GridNetHexOddr, GridNetHexMM      # noqa: F401
from .training import train_spotwise, train_gridwise, train_expression             # noqa: F401
from .multimodal_datasets import MMStackDataset, MultiModalDataset, MultiModalGridDataset  # noqa: F401
from .multimodal_datasets import SlideCountDataset                                  # noqa: F401
from .count_datasets import CountDataset, CountGridDataset                         # noqa: F401
from .image_datasets import PatchDataset, PatchGridDataset                         # noqa: F401
from .image_datasets import SlideGridDataset, SlidePatchDataset                     # noqa: F401
from . import imgprocess, metrics, optim, transforms, visium_datasets                # noqa: F401
from .visium_datasets import SpotCounts, SparseCountDataset, SparseCountGridDataset, create_visium_counts  # noqa: F401
from . import sparse_linear                                                        # noqa: F401
from .sparse_linear import SparseCountLinear, SparseCountMLP                       # noqa: F401
from . import count_pca                                                            # noqa: F401
from .count_pca import CountPCA                                                    # noqa: F401
from . import hvg                                                                  # noqa: F401
from .hvg import HighlyVariableGenes                                               # noqa: F401
from . import spatial                                                              # noqa: F401
from .spatial import SpatialAutocorr, hex_offsets, neighbor_table, edge_index, permuted_table  # noqa: F401
from . import expression                                                           # noqa: F401
from .expression import SparseMSELoss, ExpressionNet                               # noqa: F401
from .expression import ExpressionMetrics, evaluate_expression                     # noqa: F401
from .utils import all_fgd_predictions, all_fgd_predictions_device, patch_saliency  # noqa: F401
