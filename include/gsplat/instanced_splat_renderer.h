// instanced_splat_renderer.h — drop-in for src/instanced_splat_renderer.h:1-34.
//
// Same class name and methods.  The Metal handles become HIP ones:
//   initialize(void* device)  -> `device` points to an int HIP device ordinal
//                                (nullptr = device 0)
//   render(void* commandBuffer, void* drawableTexture, ...)
//                             -> commandBuffer = hipStream_t (nullptr = default
//                                stream), drawableTexture = float* device
//                                framebuffer, width*height*4 fp32 RGBA
// Everything is forwarded to the C-ABI in gsplat.h.
#pragma once

#include <string>
#include <vector>

#include "gsplat.h"
#include "gsplat/gs_math.h"

struct SplatInstance {  // instanced_splat_renderer.h:6-11 (56-B AoS record)
    float rotation[4];
    float scale[3];
    float position[3];
    float color[4];
};

class InstancedSplatRenderer {
public:
    explicit InstancedSplatRenderer(std::string filepath, const gs_options* opt = nullptr);
    ~InstancedSplatRenderer();
    InstancedSplatRenderer(const InstancedSplatRenderer&) = delete;
    InstancedSplatRenderer& operator=(const InstancedSplatRenderer&) = delete;

    bool initialize(void* device);

    void render(void* commandBuffer, void* drawableTexture, const simd_float4x4& viewMatrix,
                const simd_float4x4& projectionMatrix, float viewportWidth, float viewportHeight);

    int getPointCount() const;

    // Same, into a BGRA8Unorm drawable-format device buffer (width*height*4 B),
    // the reference's drawable pixel format (metal_renderer.mm:58).
    void renderBGRA8(void* commandBuffer, void* drawableTexture, const simd_float4x4& viewMatrix,
                     const simd_float4x4& projectionMatrix, float viewportWidth, float viewportHeight);

    // Addition (not in the reference): render() plus the accumulated depth image
    // (width*height floats in HBM) from the same composite pass (gs_render_depth).
    void renderDepth(void* commandBuffer, void* drawableTexture, void* depthTexture, const simd_float4x4& viewMatrix,
                     const simd_float4x4& projectionMatrix, float viewportWidth, float viewportHeight);

    // Addition (not in the reference): render() plus `channels` per-splat feature
    // channels composited per pixel (gs_render_features): features is the
    // getPointCount() x channels float matrix in HBM, featureTexture the
    // width*height*channels float image in HBM, channels innermost.
    void renderFeatures(void* commandBuffer, void* drawableTexture, void* featureTexture, const float* features,
                        int channels, const simd_float4x4& viewMatrix, const simd_float4x4& projectionMatrix,
                        float viewportWidth, float viewportHeight);

    // Addition (not in the reference): render() plus each splat's quantised
    // blend weight totals over the frame (gs_render_contrib): sum, count and
    // max are getPointCount()-entry arrays in HBM, mask (may be null) the
    // width*height byte image in HBM of the pixels that count; accumulate
    // combines the frame's totals into what the arrays hold.
    void renderContrib(void* commandBuffer, void* drawableTexture, const uint8_t* mask, uint64_t* sum,
                       uint32_t* count, uint32_t* max, bool accumulate, const simd_float4x4& viewMatrix,
                       const simd_float4x4& projectionMatrix, float viewportWidth, float viewportHeight);

    // Addition (not in the reference): render() plus each pixel's `slots`
    // (1..GS_MAX_ID_SLOTS) splats of largest quantised blend weight
    // (gs_render_ids): ids and q are width*height*slots uint32 images in HBM,
    // slots innermost (GS_ID_NONE / 0 in empty slots), count the width*height
    // image of the pixel's fragments with q > 0; q and count may be null.
    void renderIds(void* commandBuffer, void* drawableTexture, int slots, uint32_t* ids, uint32_t* q, uint32_t* count,
                   const simd_float4x4& viewMatrix, const simd_float4x4& projectionMatrix, float viewportWidth,
                   float viewportHeight);

    // Additions (not in the reference): the scene re-indexed on the device
    // (gs_select, gs_prune).  select: splat j of the new scene = splat index[j]
    // of the old one, index an m-entry uint32 list in HBM.  prune: the splats
    // with keep[i] != 0 stay, in order (keep: getPointCount() bytes in HBM);
    // outIndex (may be null; HBM, getPointCount() entries) receives the new ->
    // old map, *outCount (may be null; host) the new count.  Both wait for the
    // frames in flight and return true with the new scene in place; on false
    // the scene is unchanged and lastStatus() says why.
    bool select(const uint32_t* index, int64_t m);
    bool prune(const uint8_t* keep, uint32_t* outIndex, int64_t* outCount);

    // Additions (not in the reference): status of the last call, frame stats.
    gs_status lastStatus() const { return status_; }
    gs_stats lastStats() const;
    gs_handle* handle() const { return handle_; }

private:
    gs_handle* handle_ = nullptr;
    gs_status status_ = GS_OK;
};
