"""pointwise_amd -- MI355X-native conv3p (pointwise convolution) hot path of hkust-vgd/pointwise.

Only what the path needs: csrc/ (hand-written gfx950 HIP kernels + the C ABI of include/conv3p.h),
conv3p_op (host mirror of the reference's operator interface), stack (the models' conv3p layer stacks),
head, seg_head (the two models' heads), optim (the training drivers' momentum optimizer), distributed (batch sharding + RCCL all-reduce of the weight gradients),
provider (the reference providers' per-batch work as one launch over a resident data set),
scene (a room to model-sized blocks, block predictions voted back to the room's rows),
grid (a raw cloud thinned to one row per occupied voxel, voxel predictions projected back to its rows, per-voxel normals,
connected segments of the voxel labels or of a smooth surface, the clean-up of small ones, the segments' boxes, moments
and principal axes, and exact sums over them),
synth (synthetic clouds).
"""
from .conv3p_op import (Conv3pFunction, Conv3pInvalidArgument, Conv3pRuntimeError, conv3p, conv3p_autograd,
                        conv3p_grad, conv3p_layer, conv3p_layer_grad, neighbor_count, selu, selu_grad)
from .optim import MomentumOptimizer, exponential_decay, momentum_step
from .grid import (GridNormals, GridRoomSubsample, GridSegments, GridSubsample, SegmentAdjacency, SegmentGeometry,
                   SegmentPool, grid_subsample, grid_subsample_rooms)
from .provider import BatchBuffers, BatchProvider, assemble_batch
from .scene import (SceneBlocks, SceneRoomBlocks, SceneScores, SceneVotes, default_max_blocks, default_max_blocks_rooms,
                    scene_blocks, scene_blocks_rooms)
from .seg_head import SegmentationHead, class_weights_from_counts

__all__ = ["grid_subsample", "GridSubsample", "grid_subsample_rooms", "GridRoomSubsample", "GridNormals", "GridSegments", "SegmentGeometry", "SegmentAdjacency", "SegmentPool", "scene_blocks", "scene_blocks_rooms", "SceneRoomBlocks", "default_max_blocks_rooms", "SceneBlocks", "SceneVotes", "SceneScores", "default_max_blocks","BatchProvider", "BatchBuffers", "assemble_batch", "SegmentationHead", "class_weights_from_counts", "MomentumOptimizer", "exponential_decay", "momentum_step", "conv3p", "conv3p_grad", "conv3p_layer", "conv3p_layer_grad", "conv3p_autograd", "Conv3pFunction", "neighbor_count", "selu", "selu_grad",
           "Conv3pInvalidArgument", "Conv3pRuntimeError"]
