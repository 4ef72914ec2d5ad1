// tests/sim/hip_emu_grid3d/launch_3d.h -- TEST AID, force-included after hip_emu/hip/hip_runtime.h when tests/sim/map_fuse.mk
// compiles csrc/map_fuse_kernels.hip: the emulated launch (hip_emu/emu_runtime.cpp) runs 1-D and 2-D grids and leaves
// blockIdx.z = 0, gridDim.z = 1.  k_map_fuse_search takes its frame from blockIdx.z, so here a launch of a grid with z planes
// becomes z emulated launches of the 2-D grid, in stream order, and every emulated thread sets the plane it belongs to before it
// enters the kernel (blockIdx and gridDim are thread-local variables of the emulation; the threads of a workgroup are fibers of
// one OS thread and all write the same value).  The workgroups of k_map_fuse_search meet only within a plane.
#ifndef MVO_SIM_LAUNCH_3D_H
#define MVO_SIM_LAUNCH_3D_H
#undef hipLaunchKernelGGL
#define hipLaunchKernelGGL(kernel, grid, block, lds, stream, ...)                                                     \
    do {                                                                                                              \
        const dim3 g3__(grid);                                                                                        \
        for (unsigned z__ = 0; z__ < g3__.z; ++z__)                                                                   \
            emu_launch(                                                                                               \
                [=]() {                                                                                               \
                    blockIdx.z = z__;                                                                                 \
                    gridDim.z = g3__.z;                                                                               \
                    (kernel)(__VA_ARGS__);                                                                            \
                },                                                                                                    \
                dim3(g3__.x, g3__.y), dim3(block), (lds), (stream));                                                  \
    } while (0)
#endif
