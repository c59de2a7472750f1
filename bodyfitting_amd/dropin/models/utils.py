"""`from models.utils import JointMapper, smpl_to_openpose` (smplify/smplify.py:10): the joint permutation smplx applies to its
144 SMPL-X joints (`bodyfitting_amd.layout.smpl_to_openpose`) and the callable that applies it to [B, J, 3] tensors or arrays."""
from bodyfitting_amd.smplx import JointMapper, smpl_to_openpose  # noqa: F401
