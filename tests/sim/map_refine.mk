# tests/sim/map_refine.mk -- TEST AID built by tests/test_map_refine_sim.py into tests/sim/_build/ (never part of
# libmvo_hip.so): libmvo_sim_map_refine.so = the objects of libmvo_sim_map_refresh.so (map_refresh.mk) plus
# csrc/map_refine_host.cpp and csrc/map_refine_kernels.hip, compiled for x86 against hip_emu/ by the same pattern rule:
# every lane of k_map_refine runs as a fiber on the CPU.
#   make -C tests/sim -f map_refine.mk _build/libmvo_sim_map_refine.so
include map_refresh.mk
MAP_REFINE_OBJ := $(MAP_REFRESH_OBJ) _build/full/map_refine_host.cpp.o _build/full/map_refine_kernels.hip.o
_build/libmvo_sim_map_refine.so: $(MAP_REFINE_OBJ)
	$(CXX) -shared -fPIC -pthread -o $@ $^
