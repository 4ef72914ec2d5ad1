# tests/sim/map_refresh.mk -- TEST AID built by tests/test_map_refresh_sim.py into tests/sim/_build/ (never part of
# libmvo_hip.so): libmvo_sim_map_refresh.so = the objects of libmvo_sim_orb_distribute.so (orb_distribute.mk) plus
# csrc/map_refresh_host.cpp and csrc/map_refresh_kernels.hip, compiled for x86 against hip_emu/ by the same pattern rule:
# every lane of k_map_refresh runs as a fiber on the CPU.
#   make -C tests/sim -f map_refresh.mk _build/libmvo_sim_map_refresh.so
include orb_distribute.mk
MAP_REFRESH_OBJ := $(ORB_DISTRIBUTE_OBJ) _build/full/map_refresh_host.cpp.o _build/full/map_refresh_kernels.hip.o
_build/libmvo_sim_map_refresh.so: $(MAP_REFRESH_OBJ)
	$(CXX) -shared -fPIC -pthread -o $@ $^
