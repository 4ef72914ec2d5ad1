# tests/sim/window_triangulate.mk -- TEST AID built by tests/test_window_triangulate_sim.py into tests/sim/_build/ (never part of
# libmvo_hip.so): libmvo_sim_window_triangulate.so = the objects of libmvo_sim_map_fuse.so (map_fuse.mk) plus
# csrc/window_triangulate_host.cpp and csrc/window_triangulate_kernels.hip, compiled for x86 against hip_emu/ by the same pattern
# rule: every lane of k_window_epipolar_search and k_window_verify runs as a fiber on the CPU.  The emulated launch has no third
# grid dimension, so the kernel file alone is compiled with hip_emu_grid3d/launch_3d.h (unchanged) behind the runtime's header:
# one emulated 2-D launch per frame; the verification's grid has one plane.
#   make -C tests/sim -f window_triangulate.mk _build/libmvo_sim_window_triangulate.so
include map_fuse.mk
WINDOW_TRIANGULATE_OBJ := $(MAP_FUSE_OBJ) _build/full/window_triangulate_host.cpp.o _build/full/window_triangulate_kernels.hip.o
_build/full/window_triangulate_kernels.hip.o: FLAGS += -include hip_emu_grid3d/launch_3d.h
_build/full/window_triangulate_kernels.hip.o: hip_emu_grid3d/launch_3d.h $(CSRC)/guided_knn2.h
_build/full/window_triangulate_host.cpp.o: $(CSRC)/guided_knn2.h $(CSRC)/guided_match_host.h
_build/libmvo_sim_window_triangulate.so: $(WINDOW_TRIANGULATE_OBJ)
	$(CXX) -shared -fPIC -pthread -o $@ $^
