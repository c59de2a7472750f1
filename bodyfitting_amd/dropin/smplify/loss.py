from bodyfitting_amd.loss import (  # noqa: F401
    FACE_LENGTH, FACE_MAPPING, HANDS_LENGTH, SKELETON_LENGTH, angle_prior, extract_countours, gmof, multiview_keypoint_loss,
    multview_mask_loss, normal_laplacian_smoothness, normal_loss_mesh_grid, perspective_projection, point_cloud_loss_chamfer_naive,
    point_cloud_loss_mesh_grid, reprojection_loss)
