// GPU ray caster (HIP, MI355X).  Same surface as the reference's GPURaycaster
// (src/include/GPURaycaster.hpp:19-41).
#ifndef TSDF_AMD_HOST_GPU_RAYCASTER_INCLUDED
#define TSDF_AMD_HOST_GPU_RAYCASTER_INCLUDED

#include <Eigen/Core>
#include <vector>

#include "DepthImage.hpp"
#include "Raycaster.hpp"
#include "TSDFVolume.hpp"

class GPURaycaster : public Raycaster {
public:
    GPURaycaster(int width = 640, int height = 480) : Raycaster{width, height} {}

    virtual void raycast(const TSDFVolume &volume, const Camera &camera,
                         Eigen::Matrix<float, 3, Eigen::Dynamic> &vertices,
                         Eigen::Matrix<float, 3, Eigen::Dynamic> &normals) const;

    // the same plus the colour of the voxel each vertex lies in ((0, 0, 0) for misses and unobserved voxels); the volume must
    // have colour enabled (not in the reference's class)
    void raycast(const TSDFVolume &volume, const Camera &camera, Eigen::Matrix<float, 3, Eigen::Dynamic> &vertices,
                 Eigen::Matrix<float, 3, Eigen::Dynamic> &normals, std::vector<uchar3> &colours) const;

    // raycast() plus the class of the voxel each vertex lies in and (votes may be null) its votes; (TSDF_CLASS_VOID, 0) for misses and
    // unclassified voxels; the volume must have classes enabled (not in the reference's class)
    void raycast_classes(const TSDFVolume &volume, const Camera &camera, Eigen::Matrix<float, 3, Eigen::Dynamic> &vertices,
                         Eigen::Matrix<float, 3, Eigen::Dynamic> &normals, std::vector<uint16_t> &classes,
                         std::vector<uint16_t> *votes = nullptr) const;

    // raycast() with the unit gradient of the fused field at every vertex in place of the cross-product normals (which are NaN along
    // every silhouette and beside every miss): tsdf_raycast_gradient_normals_device.  Same vertices; a miss is the NaN triple (not
    // in the reference's class)
    void raycast_gradient_normals(const TSDFVolume &volume, const Camera &camera, Eigen::Matrix<float, 3, Eigen::Dynamic> &vertices,
                                  Eigen::Matrix<float, 3, Eigen::Dynamic> &normals) const;

    // ray cast, then camera-space z of every vertex rounded to uint16 mm; caller deletes the image
    DepthImage *render_to_depth_image(const TSDFVolume &volume, const Camera &camera) const;
};
#endif /* TSDF_AMD_HOST_GPU_RAYCASTER_INCLUDED */
