from .mmd import MMD, get_MMD, guassian_kernel
from .utility import logger
from .svd_transform import svd_transform
from .sampler import soga_samples
from .perturb import (bisection, diff, get_modified_adj, inner, inner_margin, linear_to_triu_idx, project,
                      to_symmetric)

__all__ = ["MMD", "get_MMD", "guassian_kernel", "logger", "svd_transform", "soga_samples", "bisection", "diff",
           "get_modified_adj", "inner", "inner_margin", "linear_to_triu_idx", "project", "to_symmetric"]
