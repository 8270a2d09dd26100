from .base import BaseGDA
from .a2gnn import A2GNN
from .grade import GRADE
from .udagcn import UDAGCN
from .adagcn import AdaGCN
from .gnn import GNN
from .dane import DANE
from .tdss import TDSS
from .specreg import SpecReg
from .dgsda import DGSDA
from .strurw import StruRW
from .sagda import SAGDA
from .cwgcn import CWGCN
from .acdne import ACDNE
from .dmgnn import DMGNN
from .asn import ASN
from .dgda import DGDA
from .jhgda import JHGDA
from .sepa import SEPA
from .soga import SOGA
from .gtrans import GTrans
from .graphcta import GraphCTA
from .kbl import KBL
from .graphata import GraphATA
from .pairalign import PairAlign

__all__ = ["BaseGDA", "A2GNN", "GRADE", "UDAGCN", "AdaGCN", "GNN", "DANE", "TDSS", "SpecReg", "DGSDA", "StruRW", "SAGDA", "CWGCN", "ACDNE", "DMGNN", "ASN", "DGDA", "JHGDA", "SEPA", "SOGA", "GTrans", "GraphCTA", "KBL", "GraphATA", "PairAlign"]
