from .linear import Linear, glorot, zeros
from .prop_gcn_conv import PropGCNConv, gcn_norm
from .gcn_conv import GCNConv
from .cached_gcn_conv import CachedGCNConv
from .ppmi_conv import PPMIConv, ppmi_edges
from .reverse_layer import GradReverse
from .attention import Attention
from .a2gnn_base import A2GNNBase, global_mean_pool
from .grade_base import GRADEBase
from .udagcn_base import UDAGCNBase
from .adagcn_base import AdaGCNBase
from .sage_gin_conv import SAGEConv, GINConv
from .gat_conv import GATConv
from .gnn_base import GNNBase
from .dgsda_base import BernProp, DGSDABase
from .reweight_gnn import GCN_reweight, GS_reweight, ReweightGNN
from .mixup_gcnconv import MixUpGCNConv
from .mixup_base import MixupBase, ShuffledEdges
from .sagda_base import SAGDABase, SAGNN, SrcGNN
from .cwgcn_base import CWGCNBase
from .acdne_base import ACDNEBase
from .asn_base import ASNBase, DiffLoss, GNNVAE, InnerProductDecoder
from .dgda_base import DGDABase
from .deepwalk_pretrain import DWPretrain
from .jhgda_base import GCNPooling, JHGDABase
from .pagerank import PageRank
from .soga_base import SOGABase
from .kbl_base import KBLBase
from .node_centric_conv import NodeCentricConv, NodeCentricMLP, Sparsemax, sparsemax
from .graphata_base import GraphATABase
from .gmm_clustering import GMMClustering

__all__ = ["Linear", "glorot", "zeros", "PropGCNConv", "gcn_norm", "GCNConv", "CachedGCNConv", "PPMIConv",
           "ppmi_edges", "GradReverse", "Attention", "A2GNNBase", "GRADEBase", "UDAGCNBase", "AdaGCNBase", "SAGEConv", "GINConv", "GATConv", "GNNBase",
           "global_mean_pool", "BernProp", "DGSDABase", "GCN_reweight", "GS_reweight", "ReweightGNN", "MixUpGCNConv", "MixupBase",
           "ShuffledEdges", "SAGDABase", "SAGNN", "SrcGNN", "CWGCNBase", "ACDNEBase", "ASNBase", "GNNVAE", "InnerProductDecoder", "DiffLoss", "DGDABase", "DWPretrain",
           "JHGDABase", "GCNPooling", "PageRank", "SOGABase", "KBLBase", "sparsemax", "Sparsemax", "NodeCentricConv", "NodeCentricMLP", "GraphATABase", "GMMClustering"]
