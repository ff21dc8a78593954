/* user_texture_probe.cl -- test program for texture reads in user shader programs (csrc/user_shader.cpp, csrc/user_texture.hip):
 * a megakernel `raygen` with the 14-parameter binding contract that, for work-item i < n (n = RTProp[1]), writes
 *   imageScratch[i]      = read_imageui(imageArray, sampler, coords[i])       coords: float4 (u, v, layer, 0), slot 8
 *   imageScratch[n + i]  = read_imageui(imageArray, texels[i])                texels: int4 (x, y, layer, 0), slot 6
 * and, from work-item 0, the image queries into imageScratch[2n] and [2n + 1].  Own code. */
__kernel void raygen(__global uint* RTProp, __global uint4* imageScratch, __global uchar* image, __global float* camData,
                     __global float* scene, __global int* meshInfo, __global int4* texels, __global uint* indexData,
                     __global float4* coords, __global float* normalData, __global float* materials,
                     image2d_array_t imageArray, sampler_t sampler, __global uint* topLevel)
{
    const uint i = get_global_id(0);
    const uint n = RTProp[1];
    if (i >= n) return;
    imageScratch[i] = read_imageui(imageArray, sampler, coords[i]);
    imageScratch[n + i] = read_imageui(imageArray, texels[i]);
    if (i == 0) {
        const int2 dim = get_image_dim(imageArray);
        imageScratch[2 * n] = (uint4)((uint)get_image_width(imageArray), (uint)get_image_height(imageArray),
                                      (uint)get_image_array_size(imageArray), 7u);
        imageScratch[2 * n + 1] = (uint4)((uint)dim.x, (uint)dim.y, 0u, 7u);
    }
}
