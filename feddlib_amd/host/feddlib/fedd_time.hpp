// Time stepping of the facade: TimeSteppingTools, TimeProblem, DAESolverInTime -- the subset the reference's unsteadyLinElas
// test runs (feddlib/problems/tests/unsteadyLinElas/main.cpp): Newmark only, linear only, one block, one rank.
//   TimeSteppingTools   feddlib/problems/Solver/TimeSteppingTools.cpp (the keys the Newmark path reads)
//   TimeProblem         feddlib/problems/abstract/TimeProblem_def.hpp (assembleMassSystem :599-663, combineSystems :359-408,
//                       updateNewmarkRhs :473-524, updateSolutionNewmarkPreviousStep :875-981)
//   DAESolverInTime     feddlib/problems/Solver/DAESolverInTime_def.hpp (advanceInTimeLinearNewmark :519-607)
// Everything else these classes do in the reference (multi-stage and multi-step schemes, adaptive steps, nonlinear loops, FSI)
// is an error here that names what is built.
#pragma once
#include "fedd_facade.hpp"

namespace FEDD {

// the square matrix of small size the reference passes time-stepping definitions and coefficients in (SmallMatrix.hpp)
template <class T>
class SmallMatrix {
public:
    SmallMatrix() : n_(0) {}
    explicit SmallMatrix(int n) : n_(n), v_((size_t)n, std::vector<T>((size_t)n, T())) {}
    SmallMatrix(int n, T value) : n_(n), v_((size_t)n, std::vector<T>((size_t)n, value)) {}
    std::vector<T>& operator[](int i) { return v_.at((size_t)i); }
    const std::vector<T>& operator[](int i) const { return v_.at((size_t)i); }
    int size() const { return n_; }
private:
    int n_;
    std::vector<std::vector<T>> v_;
};

class TimeSteppingTools {
public:
    TimeSteppingTools(ParameterListPtr_Type parameterList, Teuchos::RCP<const Teuchos::Comm<int>> comm)
        : pl_(parameterList), comm_(comm) {
        // (the constructor is handed the "Timestepping Parameter" sublist, as in the reference)
        const std::string type = pl_->get("Timestepping type", "non-adaptive");
        TEUCHOS_TEST_FOR_EXCEPTION(type != "non-adaptive", std::logic_error,
                                   "Timestepping type \"" + type + "\" is not built (\"non-adaptive\" is)");
        class_ = pl_->get("Class", "Newmark");
        dt_ = pl_->get("dt", 0.01);
        tEnd_ = pl_->get("Final time", 1.);
        beta_ = pl_->get("beta", 0.25);
        gamma_ = pl_->get("gamma", 0.5);
        TEUCHOS_TEST_FOR_EXCEPTION(dt_ <= 0., std::logic_error, "Timestepping Parameter: dt must be positive");
    }
    std::string getClass() const { return class_; }
    double get_dt() const { return dt_; }
    double get_beta() const { return beta_; }
    double get_gamma() const { return gamma_; }
    double currentTime() const { return t_; }
    int currentStep() const { return step_; }
    bool continueTimeStepping() const { return t_ + 1.e-10 < tEnd_; }       // TimeSteppingTools.cpp: t < tEnd with the same slack
    void advanceTime(bool printInfo = false) {
        t_ += dt_;
        ++step_;
        if (printInfo && comm_->getRank() == 0) std::cout << "-- time step " << step_ << " done, t = " << t_ << " --" << std::endl;
    }
private:
    ParameterListPtr_Type pl_;
    Teuchos::RCP<const Teuchos::Comm<int>> comm_;
    std::string class_;
    double dt_ = 0., tEnd_ = 0., beta_ = 0.25, gamma_ = 0.5, t_ = 0.;
    int step_ = 0;
};

// Wraps a linear single-block Problem.  The mass matrix lives in device slot 0, the problem's matrix in slot 1, the combined
// matrix is the device's system matrix; u_n, v, w live on the device (fedd_newmark_*); right-hand side, source term and
// solution are the wrapped problem's host vectors, as everywhere in this facade.
template <class SC = default_sc, class LO = default_lo, class GO = default_go, class NO = default_no>
class TimeProblem {
public:
    typedef Problem<SC, LO, GO, NO> Problem_Type;
    typedef typename Problem_Type::Matrix_Type Matrix_Type;
    typedef typename Problem_Type::MatrixPtr_Type MatrixPtr_Type;
    typedef typename Problem_Type::BlockMatrix_Type BlockMatrix_Type;
    typedef typename Problem_Type::BlockMatrixPtr_Type BlockMatrixPtr_Type;
    typedef typename Problem_Type::BlockMultiVectorPtr_Type BlockMultiVectorPtr_Type;
    typedef Teuchos::RCP<const Teuchos::Comm<int>> CommConstPtr_Type;
    static constexpr int SLOT_MASS = 0, SLOT_SYSTEM = 1;

    TimeProblem(Problem_Type& problem, CommConstPtr_Type comm) : problem_(&problem), comm_(comm) {
        TEUCHOS_TEST_FOR_EXCEPTION(comm->getSize() != 1, std::logic_error, "TimeProblem: one rank only (the Newmark device layer is one rank)");
        TEUCHOS_TEST_FOR_EXCEPTION((dynamic_cast<NonLinearProblem<SC, LO, GO, NO>*>(problem_) != nullptr), std::logic_error,
                                   "TimeProblem: nonlinear problems are not built; linear \"Newmark\" is");
    }
    void setTimeDef(const SmallMatrix<int>& def) {
        TEUCHOS_TEST_FOR_EXCEPTION(def.size() != 1, std::logic_error, "TimeProblem::setTimeDef: only a 1 x 1 definition is built (one block, \"Newmark\")");
        timeStepDef_ = def;
    }
    // TimeProblem::assembleMassSystem (:599-663): FE::assemblyMass on the variable's space, scaled by "Density" (:605, 620).
    // The problem's own matrix, still in the device's system slot after Problem::assemble, moves to slot 1 first.
    void assembleMassSystem() {
        auto sys = problem_->getSystem();
        TEUCHOS_TEST_FOR_EXCEPTION(sys.is_null() || sys->size() != 1 || !sys->blockExists(0, 0), std::logic_error,
                                   "TimeProblem: a single-block problem, assembled (Problem::assemble), is needed");
        MatrixPtr_Type K = sys->getBlock(0, 0);
        TEUCHOS_TEST_FOR_EXCEPTION(!K->isResident(), std::runtime_error, "TimeProblem: the problem's matrix is not resident on the device");
        dev_ = K->device();
        if (K->slot() < 0) {
            feddCheck(fedd_matrix_store(dev_->ctx, SLOT_SYSTEM), "fedd_matrix_store");
            K->bindSlot(dev_, SLOT_SYSTEM);
        }
        const int dofs = problem_->getDofsPerNode(0), dim = (int)problem_->getDomain(0)->getDimension();
        const double density = problem_->getParameterList()->sublist("Parameter").get("Density", 1.);
        auto map = dofs > 1 ? problem_->getDomain(0)->getMapVecFieldUnique() : problem_->getDomain(0)->getMapUnique();
        MatrixPtr_Type M = Teuchos::rcp(new Matrix_Type(map, problem_->getDomain(0)->getApproxEntriesPerRow()));
        problem_->getFEFactory()->assemblyMass(dim, problem_->getFEType(0), dofs > 1 ? "Vector" : "Scalar", M);
        M->scale(density);
        feddCheck(fedd_matrix_store(dev_->ctx, SLOT_MASS), "fedd_matrix_store");
        M->bindSlot(dev_, SLOT_MASS);
        systemMass_.reset(new BlockMatrix_Type(1));
        systemMass_->addBlock(M, 0, 0);
    }
    void setTimeParameters(const SmallMatrix<double>& massParameters, const SmallMatrix<double>& timeParameters) {
        TEUCHOS_TEST_FOR_EXCEPTION(massParameters.size() != 1 || timeParameters.size() != 1, std::logic_error, "TimeProblem: 1 x 1 parameters only");
        massParameters_ = massParameters;
        timeParameters_ = timeParameters;
    }
    // TimeProblem::combineSystems (:359-408) -> fedd_matrix_combine.  The reference combines in every step; here the combined
    // matrix is rebuilt only when the coefficients or either matrix changed since the last combine (same results)
    void combineSystems() {
        TEUCHOS_TEST_FOR_EXCEPTION(systemMass_.is_null(), std::logic_error, "TimeProblem::combineSystems: call assembleMassSystem first");
        const double cm = massParameters_[0][0], ca = timeParameters_[0][0];
        int current = 0;
        feddCheck(fedd_matrix_combine_current(dev_->ctx, SLOT_MASS, cm, SLOT_SYSTEM, ca, &current), "fedd_matrix_combine_current");
        if (current && !systemCombined_.is_null()) return;
        feddCheck(fedd_matrix_combine(dev_->ctx, SLOT_MASS, cm, SLOT_SYSTEM, ca), "fedd_matrix_combine");
        dev_->generation++;
        MatrixPtr_Type C = Teuchos::rcp(new Matrix_Type(systemMass_->getBlock(0, 0)->getMap()));
        C->bind(dev_, problem_->getDofsPerNode(0));
        systemCombined_.reset(new BlockMatrix_Type(1));
        systemCombined_->addBlock(C, 0, 0);
        fresh_ = true;
        ++combines_;
    }
    // updateSolutionNewmarkPreviousStep (:875-981) and updateNewmarkRhs (:473-524) are ONE device call, fedd_newmark_advance:
    // the first only records its arguments, the second launches (state update, then rhs <- coeff * M t) and brings the
    // right-hand side to the host vector.  Calling the second without the first is an error.
    void updateSolutionNewmarkPreviousStep(double dt, double beta, double gamma) {
        pend_ = true; pendDt_ = dt; pendBeta_ = beta; pendGamma_ = gamma;
    }
    void updateNewmarkRhs(double dt, double beta, double gamma, vec_dbl_Type coeff) {
        TEUCHOS_TEST_FOR_EXCEPTION(!pend_ || dt != pendDt_ || beta != pendBeta_ || gamma != pendGamma_, std::logic_error,
                                   "TimeProblem::updateNewmarkRhs: call updateSolutionNewmarkPreviousStep with the same dt, beta, gamma first");
        TEUCHOS_TEST_FOR_EXCEPTION(systemCombined_.is_null(), std::logic_error, "TimeProblem::updateNewmarkRhs: call combineSystems first");
        pend_ = false;
        if (!began_) {       // the start values of :913-926: u_n <- the problem's solution, v = w = 0
            feddCheck(fedd_solution_set(dev_->ctx, problem_->getSolution()->getBlock(0)->raw().data()), "fedd_solution_set");
            feddCheck(fedd_newmark_begin(dev_->ctx), "fedd_newmark_begin");
            began_ = true;
        }
        feddCheck(fedd_newmark_advance(dev_->ctx, SLOT_MASS, dt, beta, gamma, coeff.at(0)), "fedd_newmark_advance");
        feddCheck(fedd_rhs_get(dev_->ctx, problem_->getRhs()->getBlockNonConst(0)->raw().data()), "fedd_rhs_get");
    }
    void updateTime(double time) { time_ = time; }
    void assembleSourceTerm(double time) { problem_->assembleSourceTerm(time); }
    bool hasSourceTerm() const { return problem_->hasSourceTerm(); }
    BlockMultiVectorPtr_Type getSourceTerm() { return problem_->getSourceTerm(); }
    void addToRhs(BlockMultiVectorPtr_Type x) { problem_->addToRhs(x); }
    // a rebuilt matrix gets its Dirichlet rows and values (BCBuilder::set); while it stands only the values of the
    // right-hand side are set, so the preconditioner and the solver's SpMV setup stand too
    void setBoundaries(double time = .0) {
        auto bc = problem_->getBCFactory();
        TEUCHOS_TEST_FOR_EXCEPTION(bc.is_null(), std::runtime_error, "No boundary conditions added.");
        if (fresh_) bc->set(systemCombined_, problem_->getRhs(), time);
        else bc->setRHS(problem_->getRhs(), time);
    }
    // the existing LinearSolver on the combined matrix, the previous solution as the initial guess; the preconditioner is
    // built when the matrix was rebuilt and kept otherwise ("MonolithicConstPrec")
    int solve() {
        auto pl = problem_->getParameterList();
        const bool zeroGuess = pl->get("Zero Initial Guess", true);
        pl->set("Zero Initial Guess", false);
        BlockMatrixPtr_Type steady = problem_->system_;
        problem_->system_ = systemCombined_;
        LinearSolver<SC, LO, GO, NO> linSolver;
        int its = 0;
        try {
            its = linSolver.solve(problem_, Teuchos::null, fresh_ ? "Monolithic" : "MonolithicConstPrec");
        } catch (...) {
            problem_->system_ = steady;
            pl->set("Zero Initial Guess", zeroGuess);
            throw;
        }
        problem_->system_ = steady;
        pl->set("Zero Initial Guess", zeroGuess);
        fresh_ = false;
        lastRelativeResidual_ = linSolver.lastRelativeResidual;
        if (problem_->getVerbose()) std::cout << "-- time " << time_ << ": " << its << " iterations, relative residual " << lastRelativeResidual_ << std::endl;
        return its;
    }
    BlockMultiVectorPtr_Type getSolution() { return problem_->getSolution(); }
    BlockMatrixPtr_Type getSystemCombined() const { return systemCombined_; }
    BlockMatrixPtr_Type getMassSystem() const { return systemMass_; }
    Problem_Type* getUnderlyingProblem() { return problem_; }
    double getLastRelativeResidual() const { return lastRelativeResidual_; }
    int numberOfCombines() const { return combines_; }
private:
    Problem_Type* problem_;
    CommConstPtr_Type comm_;
    DeviceContextPtr dev_;
    SmallMatrix<int> timeStepDef_;
    SmallMatrix<double> massParameters_, timeParameters_;
    BlockMatrixPtr_Type systemMass_, systemCombined_;
    bool fresh_ = false, began_ = false, pend_ = false;
    double pendDt_ = 0., pendBeta_ = 0., pendGamma_ = 0., time_ = 0., lastRelativeResidual_ = 0.;
    int combines_ = 0;
};

template <class SC = default_sc, class LO = default_lo, class GO = default_go, class NO = default_no>
class DAESolverInTime {
public:
    typedef Problem<SC, LO, GO, NO> Problem_Type;
    typedef TimeProblem<SC, LO, GO, NO> TimeProblem_Type;
    typedef Teuchos::RCP<const Teuchos::Comm<int>> CommConstPtr_Type;
    typedef ExporterParaView<SC, LO, GO, NO> Exporter_Type;

    DAESolverInTime(ParameterListPtr_Type& parameterList, CommConstPtr_Type comm) : parameterList_(parameterList), comm_(comm) {}
    void defineTimeStepping(const SmallMatrix<int>& def) { timeStepDef_ = def; }
    void setProblem(Problem_Type& problem) {
        TEUCHOS_TEST_FOR_EXCEPTION((dynamic_cast<NonLinearProblem<SC, LO, GO, NO>*>(&problem) != nullptr), std::logic_error,
                                   "DAESolverInTime: time stepping of nonlinear problems is not built; the class \"Newmark\" on a linear problem is");
        problem_ = &problem;
        problemTime_.reset(new TimeProblem_Type(problem, comm_));
    }
    void setupTimeStepping() {                                          // DAESolverInTime_def.hpp: setupTimeStepping
        TEUCHOS_TEST_FOR_EXCEPTION(problemTime_.is_null(), std::logic_error, "DAESolverInTime: call setProblem first");
        checkClass();
        ParameterListPtr_Type tsl(new Teuchos::ParameterList(parameterList_->sublist("Timestepping Parameter")));
        timeSteppingTool_.reset(new TimeSteppingTools(tsl, comm_));
        problemTime_->setTimeDef(timeStepDef_);
        problemTime_->assembleMassSystem();
    }
    void advanceInTime() {
        TEUCHOS_TEST_FOR_EXCEPTION(timeSteppingTool_.is_null(), std::logic_error, "DAESolverInTime: call setupTimeStepping first");
        checkClass();
        advanceInTimeLinearNewmark();
    }
    Teuchos::RCP<TimeProblem_Type> getTimeProblem() const { return problemTime_; }
    int stepsDone() const { return timeSteppingTool_.is_null() ? 0 : timeSteppingTool_->currentStep(); }
private:
    void checkClass() const {
        const std::string cls = parameterList_->sublist("Timestepping Parameter").get("Class", "Newmark");
        TEUCHOS_TEST_FOR_EXCEPTION(cls != "Newmark", std::logic_error,
                                   "Timestepping Parameter \"Class\" = \"" + cls + "\" is not built (Singlestep, Multistep and External are not); \"Newmark\" on a linear problem is");
    }
    // DAESolverInTime::advanceInTimeLinearNewmark (:519-607), in the reference's order
    void advanceInTimeLinearNewmark() {
        const bool print = parameterList_->sublist("General").get("ParaViewExport", false);
        if (print) exportTimestep();
        TEUCHOS_TEST_FOR_EXCEPTION(timeStepDef_.size() > 1, std::runtime_error, "Newmark only implemented for systems of size 1x1.");
        const double dt = timeSteppingTool_->get_dt(), beta = timeSteppingTool_->get_beta(), gamma = timeSteppingTool_->get_gamma();
        SmallMatrix<double> massCoeff(1), problemCoeff(1);
        massCoeff[0][0] = 1.0 / (dt * dt * beta);
        problemCoeff[0][0] = 1.0;
        const double coeffSourceTerm = 1.0;
        vec_dbl_Type coeffTemp(1, 1.0);
        problemTime_->setTimeParameters(massCoeff, problemCoeff);
        while (timeSteppingTool_->continueTimeStepping()) {
            problemTime_->combineSystems();
            problemTime_->updateSolutionNewmarkPreviousStep(dt, beta, gamma);
            const double time = timeSteppingTool_->currentTime() + dt;
            problemTime_->updateTime(timeSteppingTool_->currentTime());
            problemTime_->updateNewmarkRhs(dt, beta, gamma, coeffTemp);
            if (problemTime_->hasSourceTerm()) {
                problemTime_->assembleSourceTerm(time);
                addSourceTermToRHS(coeffSourceTerm);
            }
            problemTime_->setBoundaries(time);
            problemTime_->solve();
            timeSteppingTool_->advanceTime(true);
            if (print) exportTimestep();
        }
        comm_->barrier();
        if (print && !exporter_.is_null()) exporter_->closeExporter();
    }
    void addSourceTermToRHS(double coeff) {                            // :1444-1450
        auto rhs = problemTime_->getUnderlyingProblem()->getRhs();
        rhs->update(coeff, *problemTime_->getSourceTerm(), 1.);
    }
    void exportTimestep() {
        if (exporter_.is_null()) {
            exporter_.reset(new Exporter_Type());
            auto dom = problem_->getDomain(0);
            exporter_->setup(problem_->getVariableName(0), dom->getMesh(), problem_->getFEType(0));
            exportSolution_ = problem_->getSolution()->getBlock(0);
            const int dofs = problem_->getDofsPerNode(0);
            exporter_->addVariable(exportSolution_, problem_->getVariableName(0), dofs > 1 ? "Vector" : "Scalar", dofs, dom->getMapUnique());
        }
        exporter_->save(timeSteppingTool_->currentTime());
    }
    ParameterListPtr_Type parameterList_;
    CommConstPtr_Type comm_;
    SmallMatrix<int> timeStepDef_;
    Problem_Type* problem_ = nullptr;
    Teuchos::RCP<TimeProblem_Type> problemTime_;
    Teuchos::RCP<TimeSteppingTools> timeSteppingTool_;
    Teuchos::RCP<Exporter_Type> exporter_;
    Teuchos::RCP<const MultiVector<SC, LO, GO, NO>> exportSolution_;
};

}  // namespace FEDD
