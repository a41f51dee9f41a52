// FrameDiff over the C ABI (include/tsdf_amd.h, "frame differences").
#include "FrameDiff.hpp"

#include "host_common.hpp"

namespace {

// device copies that go when the call ends, however it ends
struct DeviceArrays {
    std::vector<void *> held;
    ~DeviceArrays() {
        for (void *p : held) tsdf_device_free(p);
    }
    int make(size_t bytes, const void *host, void **out) {
        *out = nullptr;
        int rc = tsdf_device_alloc(bytes ? bytes : 4, out);
        if (rc != TSDF_OK) return rc;
        held.push_back(*out);
        return host && bytes ? tsdf_device_upload(*out, host, bytes) : TSDF_OK;
    }
};

}  // namespace

FrameDiff::FrameDiff() : m_handle(nullptr) { tsdf_host::check(tsdf_frame_diff_create(&m_handle), "Couldn't create the frame differences handle"); }

FrameDiff::~FrameDiff() { tsdf_frame_diff_destroy(m_handle); }

tsdf_frame_diff_info FrameDiff::info() const {
    tsdf_frame_diff_info i;
    tsdf_host::check(tsdf_frame_diff_get_info(m_handle, &i), "Couldn't read the frame differences info");
    return i;
}

uint64_t FrameDiff::scratch_bytes() const {
    uint64_t bytes = 0;
    tsdf_host::check(tsdf_frame_diff_scratch_bytes(m_handle, &bytes), "Couldn't read the frame differences scratch size");
    return bytes;
}

uint64_t FrameDiff::compare(const uint16_t *frame, const uint16_t *model, uint32_t width, uint32_t height, uint32_t tolerance, uint32_t quadratic,
                            std::vector<uint8_t> *states) {
    if (!frame || !model) throw std::invalid_argument("FrameDiff::compare: null frame or model");
    const size_t n = (size_t)width * height;
    if (n == 0 || width > 65535u || height > 65535u) throw std::invalid_argument("FrameDiff::compare: the image's sides are 1 .. 65535");
    DeviceArrays d;
    void *df, *dm, *ds = nullptr;
    int rc = d.make(n * sizeof(uint16_t), frame, &df);
    if (rc == TSDF_OK) rc = d.make(n * sizeof(uint16_t), model, &dm);
    if (rc == TSDF_OK && states) rc = d.make(n, nullptr, &ds);
    const tsdf_diff_params params = {tolerance, quadratic};
    if (rc == TSDF_OK) rc = tsdf_frame_diff_compare_device(m_handle, (const uint16_t *)df, (const uint16_t *)dm, width, height, &params, (uint8_t *)ds, nullptr);
    if (rc == TSDF_OK && states) {
        states->resize(n);
        rc = tsdf_device_download(states->data(), ds, n);
    }
    tsdf_host::check(rc, "Couldn't compare the frame with the model");
    return info().counts[TSDF_DIFF_NEARER];
}

std::vector<uint64_t> FrameDiff::counts() const {
    const tsdf_frame_diff_info i = info();
    return std::vector<uint64_t>(i.counts, i.counts + 5);
}

uint64_t FrameDiff::cluster(uint32_t connectivity, uint32_t depth_step, uint32_t min_pixels) {
    tsdf_host::check(tsdf_frame_diff_cluster(m_handle, connectivity, depth_step, min_pixels, nullptr), "Couldn't cluster the frame differences");
    return info().n_blobs;
}

std::vector<uint32_t> FrameDiff::pixels() const {
    std::vector<uint32_t> v((size_t)info().counts[TSDF_DIFF_NEARER]);
    tsdf_host::check(tsdf_frame_diff_download(m_handle, v.data(), nullptr, nullptr), "Couldn't download the listed pixels");
    return v;
}

std::vector<uint32_t> FrameDiff::labels() const {
    std::vector<uint32_t> v((size_t)info().counts[TSDF_DIFF_NEARER]);
    tsdf_host::check(tsdf_frame_diff_download(m_handle, nullptr, v.data(), nullptr), "Couldn't download the labels");
    return v;
}

std::vector<tsdf_diff_blob> FrameDiff::blobs() const {
    std::vector<tsdf_diff_blob> v((size_t)info().n_kept_blobs);
    tsdf_host::check(tsdf_frame_diff_download(m_handle, nullptr, nullptr, v.data()), "Couldn't download the blobs");
    return v;
}

FrameDiff::Masked FrameDiff::mask(uint32_t dilate, const uint16_t *frame, bool blob_index) {
    const tsdf_frame_diff_info i = info();
    const size_t n = (size_t)i.width * i.height;
    Masked out;
    DeviceArrays d;
    void *dm, *db = nullptr, *df = nullptr;
    int rc = d.make(n, nullptr, &dm);
    if (rc == TSDF_OK && blob_index) rc = d.make(n * sizeof(uint32_t), nullptr, &db);
    if (rc == TSDF_OK && frame) rc = d.make(n * sizeof(uint16_t), frame, &df);
    if (rc == TSDF_OK) rc = tsdf_frame_diff_mask_device(m_handle, dilate, (uint8_t *)dm, (uint32_t *)db, (const uint16_t *)df, (uint16_t *)df, nullptr);
    if (rc == TSDF_OK) rc = tsdf_frame_diff_buffers(m_handle, nullptr, nullptr, nullptr, nullptr, nullptr);   // (waits for the mask)
    if (rc == TSDF_OK && n) {
        out.mask.resize(n);
        rc = tsdf_device_download(out.mask.data(), dm, n);
        if (rc == TSDF_OK && blob_index) {
            out.blob_index.resize(n);
            rc = tsdf_device_download(out.blob_index.data(), db, n * sizeof(uint32_t));
        }
        if (rc == TSDF_OK && frame) {
            out.frame.resize(n);
            rc = tsdf_device_download(out.frame.data(), df, n * sizeof(uint16_t));
        }
    }
    tsdf_host::check(rc, "Couldn't mask the frame differences");
    return out;
}
