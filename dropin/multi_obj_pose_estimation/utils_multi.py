"""Drop-in for multi_obj_pose_estimation/utils_multi.py (`from utils_multi import *`)."""
from singleshotpose_amd.utils_multi import *  # noqa: F401,F403
from singleshotpose_amd.utils_multi import (bbox_iou, detect_multi_batched, detect_multi_region_boxes,  # noqa: F401
                                            evaluate_multi_batched, get_multi_region_boxes, match_multi_region_boxes, nms,
                                            summarize_multi)
