# tests/sim/map_fuse.mk -- TEST AID built by tests/test_map_fuse_sim.py into tests/sim/_build/ (never part of
# libmvo_hip.so): libmvo_sim_map_fuse.so = the objects of libmvo_sim_map_refine.so (map_refine.mk) plus
# csrc/map_fuse_host.cpp and csrc/map_fuse_kernels.hip, compiled for x86 against hip_emu/ by the same pattern rule:
# every lane of k_map_fuse_search runs as a fiber on the CPU.  The emulated launch has no third grid dimension, so the kernel
# file alone is compiled with hip_emu_grid3d/launch_3d.h behind the runtime's header: one emulated 2-D launch per frame.
#   make -C tests/sim -f map_fuse.mk _build/libmvo_sim_map_fuse.so
include map_refine.mk
MAP_FUSE_OBJ := $(MAP_REFINE_OBJ) _build/full/map_fuse_host.cpp.o _build/full/map_fuse_kernels.hip.o
_build/full/map_fuse_kernels.hip.o: FLAGS += -include hip_emu_grid3d/launch_3d.h
_build/full/map_fuse_kernels.hip.o: hip_emu_grid3d/launch_3d.h $(CSRC)/guided_knn2.h
_build/full/map_fuse_host.cpp.o: $(CSRC)/guided_knn2.h $(CSRC)/guided_match_host.h
_build/libmvo_sim_map_fuse.so: $(MAP_FUSE_OBJ)
	$(CXX) -shared -fPIC -pthread -o $@ $^
