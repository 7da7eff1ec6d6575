# tests/emu/ols_circular_asan_main.cpp as a stand-alone program under AddressSanitizer + UBSan, for tests/test_emu_fftconv_circular_asan.py: the host
# emulation of the circular (WRAP) real tile kernel and real line kernel on exactly sized heap blocks.  Same compiler and flags as Makefile's
# libmi355emu_asan.so rule, without -shared: the program has its own main and needs no preloaded runtime.
#   make -f ols_circular_asan.mk && ASAN_OPTIONS=detect_leaks=0 ./ols_circular_asan
CXX = /opt/rocm/lib/llvm/bin/clang++
CSRC = ../../webgpu-fft_amd/csrc
CXXFLAGS = -std=c++17 -O1 -g -DMI355_HOST_EMU -fPIC -pthread -I$(CSRC) -I../../include -Wall -Wno-unused-function
DEPS = $(wildcard $(CSRC)/*.hpp $(CSRC)/*.def $(CSRC)/*.inc) $(CSRC)/plan.cpp ols_circular_asan_main.cpp

ols_circular_asan: $(DEPS)
	$(CXX) $(CXXFLAGS) -fsanitize=address,undefined -fno-omit-frame-pointer -ftls-model=initial-exec ols_circular_asan_main.cpp $(CSRC)/plan.cpp -o $@
