# The host emulation with MI355_RT1K_EARLY_B=1 (plan.hpp: measured, not the default) for tests/test_emu_rt1k_early.py: emu_rt1k_early.cpp includes
# emu.cpp and adds the entry point that returns the group barrier counters.  Same compiler and flags as Makefile's libmi355emu.so.
#   make -f rt1k_early.mk
CXX = /opt/rocm/lib/llvm/bin/clang++
CSRC = ../../webgpu-fft_amd/csrc
CXXFLAGS = -std=c++17 -O1 -g -DMI355_HOST_EMU -DMI355_RT1K_EARLY_B=1 -fPIC -pthread -I$(CSRC) -Wall -Wno-unused-function
DEPS = $(wildcard $(CSRC)/*.hpp $(CSRC)/*.def $(CSRC)/*.inc) $(CSRC)/plan.cpp emu.cpp emu_rt1k_early.cpp

libmi355emu_early.so: $(DEPS)
	$(CXX) $(CXXFLAGS) -shared emu_rt1k_early.cpp $(CSRC)/plan.cpp -o $@
