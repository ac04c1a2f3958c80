// instanced_splat_renderer.cpp — C++ drop-in over the C-ABI
// (src/instanced_splat_renderer.h:13-34 semantics: the ctor never throws and
// leaves an empty scene on load failure (.mm:346-349); render() returns
// silently when there is nothing to draw (.mm:434-440)).
#include "gsplat/instanced_splat_renderer.h"

#include <cstdio>

InstancedSplatRenderer::InstancedSplatRenderer(std::string filepath, const gs_options* opt) {
    status_ = gs_create(filepath.c_str(), opt, &handle_);
    if (status_ != GS_OK) {
        std::fprintf(stderr, "InstancedSplatRenderer: %s\n", gs_last_error());
        handle_ = nullptr;
    }
}

InstancedSplatRenderer::~InstancedSplatRenderer() { gs_destroy(handle_); }

bool InstancedSplatRenderer::initialize(void* device) {
    if (!handle_) return false;
    int ordinal = device ? *static_cast<int*>(device) : 0;
    status_ = gs_initialize(handle_, ordinal);
    if (status_ != GS_OK) std::fprintf(stderr, "InstancedSplatRenderer::initialize: %s\n", gs_last_error());
    return status_ == GS_OK;
}

void InstancedSplatRenderer::render(void* commandBuffer, void* drawableTexture, const simd_float4x4& viewMatrix,
                                    const simd_float4x4& projectionMatrix, float viewportWidth,
                                    float viewportHeight) {
    if (!handle_ || gs_point_count(handle_) == 0 || !drawableTexture) return;
    status_ = gs_render(handle_, viewMatrix.data(), projectionMatrix.data(), (int32_t)viewportWidth,
                        (int32_t)viewportHeight, static_cast<float*>(drawableTexture), 1, commandBuffer);
}

void InstancedSplatRenderer::renderBGRA8(void* commandBuffer, void* drawableTexture, const simd_float4x4& viewMatrix,
                                         const simd_float4x4& projectionMatrix, float viewportWidth,
                                         float viewportHeight) {
    if (!handle_ || gs_point_count(handle_) == 0 || !drawableTexture) return;
    status_ = gs_render_bgra8(handle_, viewMatrix.data(), projectionMatrix.data(), (int32_t)viewportWidth,
                              (int32_t)viewportHeight, static_cast<uint8_t*>(drawableTexture), 1, commandBuffer);
}

void InstancedSplatRenderer::renderDepth(void* commandBuffer, void* drawableTexture, void* depthTexture,
                                         const simd_float4x4& viewMatrix, const simd_float4x4& projectionMatrix,
                                         float viewportWidth, float viewportHeight) {
    if (!handle_ || gs_point_count(handle_) == 0 || !drawableTexture || !depthTexture) return;
    status_ = gs_render_depth(handle_, viewMatrix.data(), projectionMatrix.data(), (int32_t)viewportWidth,
                              (int32_t)viewportHeight, static_cast<float*>(drawableTexture),
                              static_cast<float*>(depthTexture), 1, commandBuffer);
}

void InstancedSplatRenderer::renderFeatures(void* commandBuffer, void* drawableTexture, void* featureTexture,
                                            const float* features, int channels, const simd_float4x4& viewMatrix,
                                            const simd_float4x4& projectionMatrix, float viewportWidth,
                                            float viewportHeight) {
    if (!handle_ || gs_point_count(handle_) == 0 || !drawableTexture || !featureTexture) return;
    status_ = gs_render_features(handle_, viewMatrix.data(), projectionMatrix.data(), (int32_t)viewportWidth,
                                 (int32_t)viewportHeight, features, (int32_t)channels,
                                 static_cast<float*>(drawableTexture), static_cast<float*>(featureTexture), 1,
                                 commandBuffer);
}

void InstancedSplatRenderer::renderContrib(void* commandBuffer, void* drawableTexture, const uint8_t* mask,
                                           uint64_t* sum, uint32_t* count, uint32_t* max, bool accumulate,
                                           const simd_float4x4& viewMatrix, const simd_float4x4& projectionMatrix,
                                           float viewportWidth, float viewportHeight) {
    if (!handle_ || gs_point_count(handle_) == 0 || !drawableTexture || !sum || !count || !max) return;
    status_ = gs_render_contrib(handle_, viewMatrix.data(), projectionMatrix.data(), (int32_t)viewportWidth,
                                (int32_t)viewportHeight, mask, static_cast<float*>(drawableTexture), sum, count, max,
                                accumulate ? 1 : 0, 1, commandBuffer);
}

void InstancedSplatRenderer::renderIds(void* commandBuffer, void* drawableTexture, int slots, uint32_t* ids, uint32_t* q,
                                       uint32_t* count, const simd_float4x4& viewMatrix,
                                       const simd_float4x4& projectionMatrix, float viewportWidth,
                                       float viewportHeight) {
    if (!handle_ || !drawableTexture || !ids) return;
    status_ = gs_render_ids(handle_, viewMatrix.data(), projectionMatrix.data(), (int32_t)viewportWidth,
                            (int32_t)viewportHeight, (int32_t)slots, static_cast<float*>(drawableTexture), ids, q, count, 1,
                            commandBuffer);
}

bool InstancedSplatRenderer::select(const uint32_t* index, int64_t m) {
    status_ = gs_select(handle_, index, m, 1, nullptr);
    return status_ == GS_OK;
}

bool InstancedSplatRenderer::prune(const uint8_t* keep, uint32_t* outIndex, int64_t* outCount) {
    status_ = gs_prune(handle_, keep, 1, outIndex, outCount, nullptr);
    return status_ == GS_OK;
}

int InstancedSplatRenderer::getPointCount() const { return (int)gs_point_count(handle_); }

gs_stats InstancedSplatRenderer::lastStats() const {
    gs_stats s{};
    if (handle_) gs_last_stats(handle_, &s);
    return s;
}
