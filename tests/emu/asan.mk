# TEST INFRASTRUCTURE ONLY: sanitizer build of the wavefront emulator (host code only, CPU).
#   make -C tests/emu -f asan.mk
#   ASAN_OPTIONS=detect_stack_use_after_return=0:detect_leaks=0 LD_PRELOAD=$(/opt/rocm/llvm/bin/clang++ -print-file-name=libclang_rt.asan-x86_64.so) \
#     TBS_EMU_LIB=tests/emu/libmi355sat_emu_asan.so python -m pytest tests -m 'not gpu'
# clang rather than g++ so that the sanitizer line can state that it instruments no device code: -fno-gpu-sanitize
# (there is no device pass in this compile, so the flag does not change the output; clang notes it as unused).
# Under clang the kernels' __hip_atomic_* calls are the compiler's own builtins (see hip_shim.h).
CLANGXX ?= /opt/rocm/llvm/bin/clang++
SRC = ../../timberborn_support_solver_amd/csrc
FLAGS = -std=c++17 -fPIC -I. -I$(SRC) -Wall -Wno-unused-function -Wno-unused-variable -Wno-unknown-pragmas
libmi355sat_emu_asan.so: emu.cpp hip_shim.h $(SRC)/mi355sat.hip $(SRC)/device/kernels.hip.h
	$(CLANGXX) $(FLAGS) -O1 -g -fsanitize=address,undefined -fno-gpu-sanitize -fno-omit-frame-pointer -shared -o $@ emu.cpp -x c++ $(SRC)/mi355sat.hip
