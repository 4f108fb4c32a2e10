"""hiprec — MI355X-native embedding-table training hot path for beta-recsys models.

Host-side mirrors of the reference's engine modules (``beta_rec.models.{torch_engine,mf,...}``)
over the C-ABI HIP library ``libhiprec.so`` (``csrc/``, declared in ``include/hiprec.h``).
Import as ``beta_recsys_amd`` (see the shim package of that name at the repository root).
"""
__version__ = "0.1.0"

from . import _lib  # noqa: F401
from .torch_engine import HipOptimizer, ModelEngine  # noqa: F401
from .mf import MF, DeviceTripleBatcher, MFEngine, gather_rows  # noqa: F401
from .ncf import GMF, MLP, GMFEngine, MLPEngine, NeuMF, NeuMFEngine  # noqa: F401
from .lightgcn import LightGCN, LightGCNEngine  # noqa: F401
from .ngcf import NGCF, NGCFEngine  # noqa: F401
from .mixgcf import MixGCF, MixGCFEngine  # noqa: F401
from .sgl import SGL, SGLEngine  # noqa: F401
from .lcfn import LCFN, LCFNEngine  # noqa: F401
from .simgcl import SimGCL, SimGCLEngine  # noqa: F401
from .buir import BUIR_NB, BUIREngine  # noqa: F401
from .pairwise_gmf import PairwiseGMF, PairwiseGMFEngine  # noqa: F401
from .cmn import CollaborativeMemoryNetwork, cmnEngine  # noqa: F401
from .sasrec import SASRec, SASRecEngine  # noqa: F401
from .tisasrec import TiSASRec, TiSASRecEngine  # noqa: F401
from .narm import NARM, NARMEngine  # noqa: F401
from .bert4rec import BERT4Rec, BERT4RecEngine  # noqa: F401
from .caser import Caser, CaserEngine  # noqa: F401
from .gru4rec import GRU4Rec, GRU4RecEngine  # noqa: F401
from .srgnn import SRGNN, SRGNNEngine  # noqa: F401
from .triple2vec import Triple2vec, Triple2vecEngine  # noqa: F401
from .vbcar import VBCAR, VBCAREngine  # noqa: F401
from .vaecf import VAE, VAECFEngine  # noqa: F401
from .tvbr import TVBR, TVBREngine  # noqa: F401
from .ultragcn import UltraGCN, UltraGCNEngine, get_ii_constraint_mat  # noqa: F401
from .knn import ItemKNN, ItemKNNEngine, UserKNN, UserKNNEngine  # noqa: F401
from .als import ALS, ALSEngine  # noqa: F401
from .ease import EASE, EASEEngine  # noqa: F401
from .slim import SLIM, SLIMEngine  # noqa: F401
from . import eval  # noqa: F401,A004  (evaluate / predict / rank_metrics)
from . import data  # noqa: F401  (device-side loaders / negative sampling)
from .recommend import recommend  # noqa: F401  (top-K over the whole catalogue, csrc/topk.hip)
from .eval import evaluate_full  # noqa: F401
